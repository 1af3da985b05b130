#!/usr/bin/env python3
"""Cost of the device-side mosaic augmentation (csrc/mosaic.hip) at the bench shape, batch 32 x 480 x 640:
  1. wall time of ssdseg_mosaic_inputs + ssdseg_mosaic_gt from a pool of 2 x batch samples, for three mosaics -- all identity, a
     typical one (split near the middle, windows of 1 - 2 x the quadrant: datacoder.random_mosaic's defaults at probability 1), a
     zoomed-out one (every window four times its quadrant, the fill visible) -- next to ssdseg_crop_inputs + ssdseg_crop_gt for the
     identity and a zoom-out window measured in the same run: 5 warm-up calls, then `calls` back-to-back calls between two
     synchronisations;
  2. images/sec of fit() on a ResidentDataset without and with mosaic (flips and colour augmentation on in both), the method of
     scripts/crop_augment_time.py: one warm-up epoch, then every configuration measured twice, back to back.
No reference files are needed.
usage: python scripts/mosaic_augment_time.py [batch] [calls] [steps per epoch]
       python scripts/mosaic_augment_time.py [batch] [calls] [steps per epoch] plain     part 2 without mosaic only (runs on the
                                                                                         parent commit too)"""
import copy
import ctypes as C
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
import bench
import ssdseglib
from ssdseglib import datacoder as D, _engine as E, _hip as H

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
K = int(sys.argv[3]) if len(sys.argv) > 3 else 20
plain_only = len(sys.argv) > 4 and sys.argv[4] == "plain"
h, w = bench.IMAGE_SHAPE[:2]
GMAX = 64
ctx = H.Context(0)
E.set_default_context(ctx)
print(f"device: {ctx.device_name()}")

x = bench.synthetic_images(batch, 1993).astype(np.uint8)
gt, cnt, mask = bench.synthetic_ground_truth(batch, 11)
midx = mask.argmax(-1).astype(np.uint8)
gts = [gt[i, :cnt[i]] for i in range(batch)]


def timed(once):
    for _ in range(5):
        once()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        once()
    ctx.sync()
    return (time.perf_counter() - t0) / calls


if not plain_only:
    n_pool = 2 * batch
    pool_img = ctx.empty((n_pool, h, w, 3), np.uint8).upload(np.concatenate([x, x[::-1]]))
    pool_idx = ctx.empty((n_pool, h, w), np.uint8).upload(np.concatenate([midx, midx[::-1]]))
    rows = np.zeros((n_pool, GMAX, 5), np.float32)
    for i in range(n_pool):
        rows[i, :cnt[i % batch]] = gts[i % batch]
    pool_gt = ctx.empty((n_pool, GMAX, 5)).upload(rows)
    pool_cnt = ctx.empty(n_pool, np.int32).upload(np.concatenate([cnt, cnt]).astype(np.int32))
    out_img, out_idx = ctx.empty((batch, h, w, 3), np.uint8), ctx.empty((batch, h, w), np.uint8)
    out_gt, out_cnt, out_flip = ctx.empty((batch, GMAX, 5)), ctx.empty(batch, np.int32), ctx.empty(batch, np.uint8)
    index = np.random.default_rng(3).permutation(n_pool)[:batch].astype(np.int32)
    flip = (np.arange(batch) % 2).astype(np.uint8)
    fill = (C.c_uint8 * 3)(124, 116, 104)
    mb = batch * h * w * (3 + 1) * 2 / 1e6
    typical = D.random_mosaic(np.random.default_rng(5), batch, h, w, probability=1.0)
    identity = D.random_mosaic(np.random.default_rng(5), batch, h, w, probability=0.0)
    quads = np.array([typical.quadrants(n, h, w) for n in range(batch)], np.float32)                 # (batch, 4, (qx, qy, qw, qh))
    far = np.stack([-1.5 * quads[..., 2], -1.5 * quads[..., 3], 4 * quads[..., 2], 4 * quads[..., 3]], axis=-1)
    zoomed_out = D.Mosaic(typical.index4, typical.split, far).check(h, w)
    for name, mosaic in (("all identity", identity), ("typical", typical), ("zoomed out", zoomed_out)):
        sources = np.ascontiguousarray(index[mosaic.index4], np.int32)                              # positions -> pool slots
        lists = (sources.ctypes.data, mosaic.split.ctypes.data, mosaic.windows.ctypes.data_as(C.POINTER(C.c_float)))

        def once():
            ctx.call("ssdseg_mosaic_inputs", pool_img, pool_idx, n_pool, *lists, fill, 0, flip.ctypes.data, out_flip, out_img, out_idx, batch, h, w)
            ctx.call("ssdseg_mosaic_gt", pool_gt, pool_cnt, n_pool, *lists, out_gt, out_cnt, batch, GMAX, h, w)

        dt = timed(once)
        print(f"ssdseg_mosaic_inputs + ssdseg_mosaic_gt {batch}x{h}x{w}, {name:12s}: {dt * 1e3:.3f} ms/call (wall, {calls} back-to-back calls; "
              f"{mb:.0f} MB written + as many output-sized bytes read = {mb / 1e3 / dt:.0f} GB/s effective), rows kept {int(out_cnt.download().sum())}")
    for name, window in (("all identity", (0, 0, w, h)), ("zoom-out", (-w / 2, -h / 2, 2 * w, 2 * h))):
        win = np.tile(np.array(window, np.float32), (batch, 1))
        wp = win.ctypes.data_as(C.POINTER(C.c_float))

        def once():
            ctx.call("ssdseg_crop_inputs", pool_img, pool_idx, n_pool, index.ctypes.data, wp, fill, 0, flip.ctypes.data, out_flip, out_img, out_idx,
                     batch, h, w)
            ctx.call("ssdseg_crop_gt", pool_gt, pool_cnt, n_pool, index.ctypes.data, wp, out_gt, out_cnt, batch, GMAX, h, w)

        dt = timed(once)
        print(f"ssdseg_crop_inputs   + ssdseg_crop_gt   {batch}x{h}x{w}, {name:12s}: {dt * 1e3:.3f} ms/call (the crop, same run, same method), "
              f"rows kept {int(out_cnt.download().sum())}")
    del pool_img, pool_idx, pool_gt, pool_cnt, out_img, out_idx, out_gt, out_cnt, out_flip

boxes, model = bench.build_full_model()
enc = ssdseglib.datacoder.DataEncoderDecoder(
    4, bench.IMAGE_SHAPE[:2], xmin_boxes_default=boxes.get_boxes_coordinates_xmin('ssd'), ymin_boxes_default=boxes.get_boxes_coordinates_ymin('ssd'),
    xmax_boxes_default=boxes.get_boxes_coordinates_xmax('ssd'), ymax_boxes_default=boxes.get_boxes_coordinates_ymax('ssd'),
    iou_threshold=0.525, standard_deviations_centroids_offsets=bench.STDS)
enc = copy.copy(enc)
enc.augmentation_horizontal_flip = True
os.environ["SSDSEG_FIT_OVERLAP"] = "1"
configs = [("without mosaic", {})]
if not plain_only:
    configs.append(("with mosaic", dict(mosaic=dict(probability=0.5, fill=(124, 116, 104)))))
medians = {}
for name, kw in configs:
    ds = ssdseglib.datacoder.ResidentDataset(enc, capacity=K * batch, batch_size=batch, rgb_augmentation=True, seed=1993, **kw)
    for k in range(K):
        for i in range(batch):
            ds.append(x[i], midx[i], gts[i])
    model.fit(ds, epochs=1)
    rates = []
    for _ in range(2):                                   # twice, back to back
        ctx.sync()
        t0 = time.perf_counter()
        model.fit(ds, epochs=1)
        rates.append(K * batch / (time.perf_counter() - t0))
    medians[name] = rates
    print(f"fit() on a ResidentDataset, batch {batch}, {K} steps/epoch, flips + colour augmentation, {name:14s}: "
          f"{rates[0]:.1f} and {rates[1]:.1f} images/sec (spread {100 * abs(rates[0] - rates[1]) / np.mean(rates):.2f} %)")
    del ds
if len(medians) == 2:
    a, b = medians["without mosaic"], medians["with mosaic"]
    print(f"with / without mosaic: {100 * (np.mean(b) / np.mean(a) - 1):+.2f} % (means of the two runs)")
