#!/usr/bin/env python3
"""Time of the two fused detection losses at the bench shape, batch 32 x 9600 anchors x 4 classes, all four outputs requested:
`ssdseg_det_loss` (softmax cross-entropy with batch-global 3:1 hard-negative mining; its code is the parent commit's) against
`ssdseg_det_loss_focal` (focal loss, no selection), both with the smooth-L1 localization loss fused in.

Method: seeded inputs built like the parity tests' (softmax of logits in [0, 6], 1 % positive anchors); 20 warm-up calls of each
entry; then `repeats` windows per entry, the two entries alternating, each window `calls` back-to-back calls between two HIP
events on the context's stream; per-call time = window / calls.  Reported: median, minimum, maximum and the quartiles of the
windows of each entry, and the kernel launches of one call of each (the library's own launch registry; memsets are not in it).
usage: python scripts/det_loss_time.py [batch] [anchors] [calls] [repeats] [--out FILE] [--commit TEXT]"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
from ssdseglib import _hip as H

args = sys.argv[1:]
opts = {}
for flag in ("--out", "--commit"):
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

rng = np.random.default_rng(1993)
logits = rng.uniform(0, 6, (b, a, 4))
e = np.exp(logits - logits.max(-1, keepdims=True))
p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
cls = np.where(rng.uniform(size=(b, a)) < 0.01, rng.integers(1, 4, (b, a)), 0)
y = np.eye(4, dtype=np.float32)[cls]
yb = (rng.normal(0, 2, (b, a, 4)) * (cls > 0)[..., None]).astype(np.float32)
pb = rng.uniform(0, 6, (b, a, 4)).astype(np.float32)

ctx = H.Context(0)
device = ctx.device_name()
ins = [ctx.array(v) for v in (y, p, yb, pb)]
outs = [ctx.empty(b), ctx.empty(b), ctx.empty((b, a, 4)), ctx.empty((b, a, 4))]
alpha = (C.c_float * 4)(0.25, 1.0, 0.75, 0.5)
scale = 1.0 / b
entries = {
    "ssdseg_det_loss": lambda: ctx.call("ssdseg_det_loss", *ins, b, a, 4, scale, *outs, None),
    "ssdseg_det_loss_focal": lambda: ctx.call("ssdseg_det_loss_focal", *ins, b, a, 4, alpha, 2.0, scale, scale, *outs),
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

lines = [f"Fused detection losses at {b} x {a} x 4, fp32, all four outputs (both losses, d_logits, d_boxes), one GPU.",
         f"Command: python scripts/det_loss_time.py {b} {a} {calls} {repeats}",
         f"commit: {commit}",
         f"device: {device}",
         f"{repeats} windows per entry, the entries alternating; a window = {calls} back-to-back calls between two HIP events; microseconds per call",
         ""]
stats = {}
for name, w in windows.items():
    w = np.asarray(w)
    q1, med, q3 = np.percentile(w, [25, 50, 75])
    stats[name] = (med, w.min(), w.max(), q1, q3)
    n = sum(launches[name].values())
    lines.append(f"{name:22s}: median {med:8.2f} us   min {w.min():8.2f}   max {w.max():8.2f}   quartiles {q1:8.2f} / {q3:8.2f}   "
                 f"kernel launches per call {n}" + (" (+ 2 memsets)" if name == "ssdseg_det_loss" else ""))
for name in entries:
    lines.append(f"  launches of {name}: " + ", ".join(f"{k.split('(')[0]} x{v}" for k, v in sorted(launches[name].items())))
mined, focal = stats["ssdseg_det_loss"], stats["ssdseg_det_loss_focal"]
spread = mined[4] - mined[3]
lines += ["",
          f"run-to-run spread of the yardstick (interquartile range of the mined call's windows): {spread:.2f} us; full range {mined[2] - mined[1]:.2f} us",
          f"focal - mined, medians: {focal[0] - mined[0]:+.2f} us ({100 * (focal[0] / mined[0] - 1):+.1f} %)",
          "requirement (focal not slower than mined beyond that spread): " + ("met" if focal[0] <= mined[0] + spread else "NOT met")]
text = "\n".join(lines) + "\n"
print(text, end="")
if "--out" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as f:
        f.write(text)
