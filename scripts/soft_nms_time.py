#!/usr/bin/env python3
"""Time of `ssdseg_combined_nms_soft` (Gaussian Soft-NMS, sigma 0.5) against `ssdseg_combined_nms` (the hard NMS; its kernels are
the parent commit's) on decoded boxes at the bench shape, batch 32 x 9600 anchors x 4 classes, boxes_iou_threshold 0.5.

Limits (per class / per image): 10 / 20 as scripts/eval_path_time.py uses, and 100 / 200.  Inputs, seeded: offsets ~ U[0, 6) on
the model's anchors as bench.py draws them, with near-uniform probabilities (softmax of 0.3 N(0, 1), labels_probability_threshold
0.05: every anchor of every class is a candidate and stays one for many rounds) and with peaked, trained-like ones (softmax of
3 N(0, 1), threshold 0.3).  To say where a difference comes from, both entries are also timed at boxes_iou_threshold 0: every
overlapping candidate then dies by the hard step, so the soft kernel keeps its score array but never reaches the double exp.

Method: 10 warm-up calls of each entry; then `repeats` windows per entry, the entries alternating, each window `calls` back-to-back
calls between two HIP events on the context's stream; per-call time = window / calls.  The hard entry runs twice in every round
(a twin): the difference of the twins' medians and the twin's own max - min are the yardstick's noise.  Last, ten calls of each entry
with every launch between its own events (the library's launch registry) say which kernel the time belongs to.
usage: python scripts/soft_nms_time.py [batch] [calls] [repeats] [--out FILE] [--commit TEXT]"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
import bench
from ssdseglib import _hip as H

args = sys.argv[1:]
opts = {}
for flag in ("--out", "--commit"):
    if flag in args:
        i = args.index(flag)
        opts[flag] = args[i + 1]
        del args[i:i + 2]
b = int(args[0]) if len(args) > 0 else 32
calls = int(args[1]) if len(args) > 1 else 10
repeats = int(args[2]) if len(args) > 2 else 30
commit = opts.get("--commit")
if commit is None:
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        commit = "unknown (not a git checkout)"
SIGMA, IOU_THR = 0.5, 0.5

boxes = bench.default_boxes()
cent = np.stack([boxes.get_boxes_coordinates_center_x('ssd'), boxes.get_boxes_coordinates_center_y('ssd'),
                 boxes.get_boxes_coordinates_width('ssd'), boxes.get_boxes_coordinates_height('ssd')], axis=1).astype(np.float32)
a, c = cent.shape[0], 4
rng = np.random.default_rng(1993)


def softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


INPUTS = {"near-uniform": (softmax(0.3 * rng.standard_normal((b, a, c))), 0.05), "peaked": (softmax(3.0 * rng.standard_normal((b, a, c))), 0.3)}
LIMITS = [(10, 20), (100, 200)]

ctx = H.Context(0)
device = ctx.device_name()
corners = ctx.empty((b, a, 4))
ctx.call("ssdseg_decode_boxes", ctx.array(rng.uniform(0, 6, (b, a, 4)).astype(np.float32)), ctx.array(cent), b, a, (C.c_float * 4)(*bench.STDS), corners)
valid = ctx.empty(b, np.int32)
start, stop = ctx.event(), ctx.event()
lines = [f"Soft-NMS (sigma {SIGMA}) against the hard NMS at {b} x {a} x {c}, fp32, boxes_iou_threshold {IOU_THR}, one GPU.",
         f"Command: python scripts/soft_nms_time.py {b} {calls} {repeats}",
         f"commit: {commit}",
         f"device: {device}",
         f"{repeats} windows per entry, the entries alternating; a window = {calls} back-to-back calls between two HIP events; microseconds per call",
         "hard twin: the hard entry a second time in every round; 'iou 0' rows: boxes_iou_threshold 0 (the soft kernel never reaches its exp)",
         ""]

for name, (probs, score_thr) in INPUTS.items():
    d_probs = ctx.array(probs)
    for per_class, per_image in LIMITS:
        out = ctx.empty((b, per_image, 6))
        hard = lambda thr=IOU_THR: ctx.call("ssdseg_combined_nms", corners, d_probs, b, a, c, per_class, per_image, thr, score_thr, out, valid)
        soft = lambda thr=IOU_THR: ctx.call("ssdseg_combined_nms_soft", corners, d_probs, b, a, c, per_class, per_image, thr, score_thr, SIGMA, out, valid)
        entries = {"hard": hard, "hard twin": hard, "soft": soft, "hard, iou 0": lambda: hard(0.0), "soft, iou 0": lambda: soft(0.0)}
        kept = {}
        for label, fn in entries.items():
            for _ in range(10):
                fn()
            ctx.sync()
            kept[label] = float(valid.download().mean())
        windows = {label: [] for label in entries}
        for _ in range(repeats):
            for label, fn in entries.items():
                start.record()
                for _ in range(calls):
                    fn()
                stop.record()
                ctx.sync()
                windows[label].append(start.elapsed_ms(stop) / calls * 1e3)
        med = {label: float(np.median(w)) for label, w in windows.items()}
        split = {}
        for label in ("hard", "soft"):                       # per kernel, bracketed by events, in 10 calls of their own
            ctx.timing(True)
            ctx.timing_reset()
            for _ in range(10):
                entries[label]()
            ctx.sync()
            split[label] = ", ".join(f"{k.split('(')[0]} {1e3 * v['ms'] / v['count']:.1f}" for k, v in sorted(ctx.timing_report().items()))
            ctx.timing(False)
        candidates = float((probs > np.float32(score_thr)).sum()) / (b * c)
        lines.append(f"{name} probabilities, labels_probability_threshold {score_thr}, limits {per_class} / {per_image}: "
                     f"{candidates:.0f} candidates per class and image at the start")
        for label, w in windows.items():
            lines.append(f"  {label:12s}: median {med[label]:9.2f} us   min {min(w):9.2f}   max {max(w):9.2f}   detections per image {kept[label]:.1f}")
        twin = windows["hard twin"]
        lines.append(f"  noise: |hard - hard twin| medians {abs(med['hard'] - med['hard twin']):.2f} us; the twin's own max - min {max(twin) - min(twin):.2f} us")
        lines.append(f"  soft / hard, medians: {med['soft'] / med['hard']:.2f}x ({med['soft'] - med['hard']:+.2f} us);  "
                     f"at iou 0 (no exp): {med['soft, iou 0'] / med['hard, iou 0']:.2f}x ({med['soft, iou 0'] - med['hard, iou 0']:+.2f} us)")
        lines += [f"  kernels of one {label} call, us (each launch between its own events): {split[label]}" for label in split]
        lines.append("")
text = "\n".join(lines)
print(text, end="")
if "--out" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as f:
        f.write(text)
