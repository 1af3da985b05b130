#!/usr/bin/env python3
"""What the IoU-family box regression loss adds to the detection losses at the bench shape, batch 32 x 9600 anchors x 4 classes.
Yardstick: `ssdseg_det_loss_focal` with all four outputs (focal confidence loss fused with the smooth-L1 localization loss; the
parent commit's code).  Against it the pair the engine issues with `losses.iou_localization_loss`: `ssdseg_det_loss_focal` with
both localization outputs NULL, then `ssdseg_loc_loss_iou` (GIoU, smooth_l1_weight 1) writing loc_loss and d_boxes.

Method: seeded inputs (softmax of logits in [0, 6], 1 % box-carrying anchors with targets of positive decoded size against the
model's default boxes, predictions = targets + N(0, 0.8)); 20 warm-up calls of each entry; then `repeats` windows per entry, the
two entries alternating, each window `calls` back-to-back calls between two HIP events on the context's stream; per-call time =
window / calls.  Reported: median, minimum, maximum and the quartiles of the windows of each entry, the kernel launches of one
call of each (the library's own launch registry), the pair's extra microseconds over the yardstick next to the yardstick's
interquartile range, and -- with --step-ms, the time of one `bench.py` training step measured in the same sitting -- that
extra as a share of the step.
usage: python scripts/loc_iou_time.py [batch] [anchors] [calls] [repeats] [--out FILE] [--commit TEXT] [--step-ms MS]"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
from ssdseglib import _hip as H
from ssdseglib.boxes import DefaultBoundingBoxes

args = sys.argv[1:]
opts = {}
for flag in ("--out", "--commit", "--step-ms"):
    if flag in args:
        i = args.index(flag)
        opts[flag] = args[i + 1]
        del args[i:i + 2]
b = int(args[0]) if len(args) > 0 else 32
a = int(args[1]) if len(args) > 1 else 9600
calls = int(args[2]) if len(args) > 2 else 20
repeats = int(args[3]) if len(args) > 3 else 50
commit = opts.get("--commit")
if commit is None:
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        commit = "unknown (not a git checkout)"

STDS = (0.1, 0.1, 0.2, 0.2)
boxes = DefaultBoundingBoxes(feature_maps_shapes=((30, 40), (15, 20), (8, 10), (4, 5)), centers_padding_from_borders_percentage=(0.025, 0.05, 0.075, 0.1),
                             boxes_scales=(0.15, 0.95), additional_square_box=True)
boxes.rescale_boxes_coordinates(image_shape=(480, 640))
full = np.stack([np.asarray(getattr(boxes, f"get_boxes_coordinates_{k}")("ssd"), np.float32).reshape(-1)
                 for k in ("center_x", "center_y", "width", "height")], axis=1)
anchors = np.ascontiguousarray(full[(np.arange(a) * full.shape[0]) // a])      # all 9600 of them at the default shape

rng = np.random.default_rng(1993)
logits = rng.uniform(0, 6, (b, a, 4))
e = np.exp(logits - logits.max(-1, keepdims=True))
p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
cls = np.where(rng.uniform(size=(b, a)) < 0.01, rng.integers(1, 4, (b, a)), 0)
y = np.eye(4, dtype=np.float32)[cls]
yb = np.concatenate([rng.uniform(-3, 3, (b, a, 2)), np.log1p(rng.uniform(0.3, 3.0, (b, a, 2))) / 0.2], axis=-1)
yb = (yb * (cls > 0)[..., None]).astype(np.float32)
pb = (yb + rng.normal(0, 0.8, (b, a, 4))).astype(np.float32)

ctx = H.Context(0)
device = ctx.device_name()
ins = [ctx.array(v) for v in (y, p, yb, pb)]
d_anchors = ctx.array(anchors)
conf, loc, dlog, dbox = ctx.empty(b), ctx.empty(b), ctx.empty((b, a, 4)), ctx.empty((b, a, 4))
alpha = (C.c_float * 4)(0.25, 1.0, 0.75, 0.5)
stds = (C.c_float * 4)(*STDS)
scale = 1.0 / b
YARD, PAIR = "focal, four outputs", "focal, loc NULL + loc_iou"


def pair():
    ctx.call("ssdseg_det_loss_focal", *ins, b, a, 4, alpha, 2.0, scale, scale, conf, None, dlog, None)
    ctx.call("ssdseg_loc_loss_iou", ins[2], ins[3], d_anchors, stds, b, a, 1, 1.0, scale, loc, dbox)


entries = {
    YARD: lambda: ctx.call("ssdseg_det_loss_focal", *ins, b, a, 4, alpha, 2.0, scale, scale, conf, loc, dlog, dbox),
    PAIR: pair,
}

launches = {}
for name, fn in entries.items():
    for _ in range(20):
        fn()
    ctx.sync()
    ctx.timing(True)
    ctx.timing_reset()
    fn()
    ctx.sync()
    launches[name] = {k: v["count"] for k, v in ctx.timing_report().items()}
    ctx.timing(False)

start, stop = ctx.event(), ctx.event()
windows = {name: [] for name in entries}
for _ in range(repeats):
    for name, fn in entries.items():
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        ctx.sync()
        windows[name].append(start.elapsed_ms(stop) / calls * 1e3)

lines = [f"Detection losses at {b} x {a} x 4, fp32, all four outputs (both losses, d_logits, d_boxes), one GPU.",
         f"Command: python scripts/loc_iou_time.py {b} {a} {calls} {repeats}" + (f" --step-ms {opts['--step-ms']}" if "--step-ms" in opts else ""),
         f"commit: {commit}",
         f"device: {device}",
         f"{YARD}: ssdseg_det_loss_focal (focal + smooth-L1, the parent commit's code)",
         f"{PAIR}: ssdseg_det_loss_focal with loc_loss = d_boxes = NULL, then ssdseg_loc_loss_iou (GIoU, smooth_l1_weight 1)",
         f"{repeats} windows per entry, the entries alternating; a window = {calls} back-to-back calls between two HIP events; microseconds per call",
         ""]
stats = {}
for name, w in windows.items():
    w = np.asarray(w)
    q1, med, q3 = np.percentile(w, [25, 50, 75])
    stats[name] = (med, w.min(), w.max(), q1, q3)
    lines.append(f"{name:26s}: median {med:8.2f} us   min {w.min():8.2f}   max {w.max():8.2f}   quartiles {q1:8.2f} / {q3:8.2f}   "
                 f"kernel launches per call {sum(launches[name].values())}")
for name in entries:
    lines.append(f"  launches of {name}: " + ", ".join(f"{k.split('(')[0]} x{v}" for k, v in sorted(launches[name].items())))
yard, both = stats[YARD], stats[PAIR]
extra = both[0] - yard[0]
lines += ["",
          f"run-to-run spread of the yardstick (interquartile range of its windows): {yard[4] - yard[3]:.2f} us; full range {yard[2] - yard[1]:.2f} us",
          f"pair - yardstick, medians: {extra:+.2f} us ({100 * (both[0] / yard[0] - 1):+.1f} %)"]
if "--step-ms" in opts:
    step_ms = float(opts["--step-ms"])
    lines.append(f"share of one bench.py training step ({step_ms:.2f} ms, batch {b}, measured in the same sitting): {100 * extra / (step_ms * 1e3):.3f} %")
text = "\n".join(lines) + "\n"
print(text, end="")
if "--out" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as f:
        f.write(text)
