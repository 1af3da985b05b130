#!/usr/bin/env python3
"""Time of the mask head's training pair (forward with the loss, no stored probabilities, + backward) at the bench shape, batch
32 x 120 x 160 logits up-sampled x4 to 480 x 640: the cross-entropy pair (`ssdseg_mask_head_fwd` + `ssdseg_mask_head_bwd`)
against the bootstrapped pair (`ssdseg_mask_head_fwd_bootstrap` + `ssdseg_mask_head_bwd_bootstrap`, keep_fraction 0.25), and the
bootstrapped pair's parts: the forward that stores the pixel losses, the four select passes, the sum and the backward.

Method: seeded inputs built like the parity tests' (logits normal(0, 2), uniform classes); 20 warm-up calls of each pair; then
`repeats` windows per pair, the two pairs alternating, each window `calls` back-to-back pairs between two HIP events on the
context's stream; per-pair time = window / calls.  The parts come from the library's own launch registry (one HIP-event bracket
per launch, mean over `calls` pairs; the histogram memset is not in it), so they carry the bracket's overhead and do not add up
to the window figure exactly.
usage: python scripts/mask_bootstrap_time.py [batch] [h] [w] [calls] [repeats] [--out FILE] [--commit TEXT]"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
from ssdseglib import _hip as H
from ssdseglib import losses as LS

args = sys.argv[1:]
opts = {}
for flag in ("--out", "--commit"):
    if flag in args:
        i = args.index(flag)
        opts[flag] = args[i + 1]
        del args[i:i + 2]
n = int(args[0]) if len(args) > 0 else 32
h = int(args[1]) if len(args) > 1 else 120
w = int(args[2]) if len(args) > 2 else 160
calls = int(args[3]) if len(args) > 3 else 20
repeats = int(args[4]) if len(args) > 4 else 30
f, fraction = 4, 0.25
commit = opts.get("--commit")
if commit is None:
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        commit = "unknown (not a git checkout)"

rng = np.random.default_rng(1993)
hw = h * f * w * f
keep = LS.bootstrap_keep(fraction, hw)
ctx = H.Context(0)
device = ctx.device_name()
logits = ctx.array(rng.normal(0, 2, (n, h, w, 4)).astype(np.float32))
y = ctx.empty((n, h * f, w * f, 4))
for b in range(n):          # one image at a time: 39 MB of one-hot rows per image on the host
    rows = np.eye(4, dtype=np.float32)[rng.integers(0, 4, (h * f, w * f))]
    ctx.borrow(y.ptr + b * rows.nbytes, rows.shape, np.float32, owner=y).upload(rows)
cw = (C.c_float * 4)(0.05, 0.575, 0.135, 0.24)
loss, g = ctx.empty(n), ctx.empty((n, h, w, 4))
pixel_loss, thresh, kept = ctx.empty((n, hw)), ctx.empty(n), ctx.empty(n, np.int32)
scale = 1.0 / n


def ce_pair():
    ctx.call("ssdseg_mask_head_fwd", logits, n, h, w, 4, f, f, y, cw, None, loss)
    ctx.call("ssdseg_mask_head_bwd", logits, n, h, w, 4, f, f, y, cw, scale, g)


def bootstrap_pair():
    ctx.call("ssdseg_mask_head_fwd_bootstrap", logits, n, h, w, 4, f, f, y, cw, keep, None, pixel_loss, thresh, kept, loss)
    ctx.call("ssdseg_mask_head_bwd_bootstrap", logits, n, h, w, 4, f, f, y, cw, pixel_loss, thresh, scale, g)


pairs = {"cross-entropy pair": ce_pair, "bootstrapped pair": bootstrap_pair}
parts = {}
for name, fn in pairs.items():
    for _ in range(20):
        fn()
    ctx.sync()
    ctx.timing(True)
    ctx.timing_reset()
    for _ in range(calls):
        fn()
    ctx.sync()
    parts[name] = {k: (v["count"] // calls, v["ms"] / calls * 1e3, v["bytes"] / calls) for k, v in ctx.timing_report().items()}
    ctx.timing(False)
kept_host = kept.download()

start, stop = ctx.event(), ctx.event()
windows = {name: [] for name in pairs}
for _ in range(repeats):
    for name, fn in pairs.items():
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        ctx.sync()
        windows[name].append(start.elapsed_ms(stop) / calls * 1e3)

lines = [f"Mask head training pair (forward with loss, no stored probabilities, + backward) at {n} x {h} x {w} logits x{f} -> {h * f} x {w * f}, fp32, one GPU.",
         f"Command: python scripts/mask_bootstrap_time.py {n} {h} {w} {calls} {repeats}",
         f"commit: {commit}   (the cross-entropy pair's forward kernel is the parent commit's instruction for instruction; its backward kernels",
         "         gained two NULL pointer arguments and a mode test)",
         f"device: {device}",
         f"bootstrapped: keep_fraction {fraction}, keep = {keep} of {hw} pixels per image; kept per image {int(kept_host.min())} ... {int(kept_host.max())}",
         f"{repeats} windows per pair, the pairs alternating; a window = {calls} back-to-back pairs between two HIP events; microseconds per pair",
         ""]
stats = {}
for name, win in windows.items():
    win = np.asarray(win)
    q1, med, q3 = np.percentile(win, [25, 50, 75])
    stats[name] = med
    lines.append(f"{name:20s}: median {med:8.2f} us   min {win.min():8.2f}   max {win.max():8.2f}   quartiles {q1:8.2f} / {q3:8.2f}")
lines.append("")
for name in pairs:
    lines.append(f"launches of one {name} (launch registry: launches, mean microseconds per pair, algorithmic MB, GB/s):")
    for k, (count, us, nbytes) in sorted(parts[name].items(), key=lambda kv: -kv[1][1]):
        lines.append(f"  {k.split('(')[0] if not k.startswith('(') else k:52s} x{count}   {us:8.2f} us   {nbytes / 1e6:8.1f} MB   {nbytes / us / 1e3 if us > 0 else 0:7.0f} GB/s")
    lines.append(f"  {'sum':52s}      {sum(v[1] for v in parts[name].values()):8.2f} us")
ratio = stats["bootstrapped pair"] / stats["cross-entropy pair"]
lines += ["", f"bootstrapped / cross-entropy, medians: {ratio:.3f}x  ({stats['bootstrapped pair'] - stats['cross-entropy pair']:+.2f} us per step)"]
text = "\n".join(lines) + "\n"
print(text, end="")
if "--out" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as fh:
        fh.write(text)
