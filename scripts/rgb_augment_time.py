#!/usr/bin/env python3
"""Wall time of ssdseg_rgb_augment (the colour augmentation of a compact batch: stats, means and apply kernels) at the bench
shape, batch 32 x 480 x 640, half the images mirrored.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
usage: python scripts/rgb_augment_time.py [batch] [calls]"""
import ctypes as C
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
import bench
from ssdseglib import _hip as H

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
h, w = bench.IMAGE_SHAPE[:2]
ctx = H.Context(0)
img = ctx.empty((batch, h, w, 3), np.uint8).upload(bench.synthetic_images(batch, 1993).astype(np.uint8))
flip = ctx.empty(batch, np.uint8).upload((np.arange(batch) % 2).astype(np.uint8))
means, out = ctx.empty((batch, 3)), ctx.empty((batch, h, w, 3))
draws = (C.c_float * 4)(0.03, 1.02, 0.95, -0.04)
for _ in range(5):
    ctx.call("ssdseg_rgb_augment", img, flip, draws, means, out, batch, h, w)
ctx.sync()
t0 = time.perf_counter()
for _ in range(calls):
    ctx.call("ssdseg_rgb_augment", img, flip, draws, means, out, batch, h, w)
ctx.sync()
dt = (time.perf_counter() - t0) / calls
mb = batch * h * w * (3 + 12) / 1e6
print(f"ssdseg_rgb_augment {batch}x{h}x{w}: {dt * 1e3:.3f} ms/call (wall, {calls} back-to-back calls; {mb:.0f} MB in + out "
      f"= {mb / 1e3 / dt:.0f} GB/s effective)")
