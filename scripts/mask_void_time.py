#!/usr/bin/env python3
"""Time of the void-pixel variants of the mask head's losses and metric against their plain twins, and of the fused evaluation pass
(`ssdseg_eval_mask_scores`: soft Jaccard + confusion counts) against `ssdseg_eval_mask_jaccard`, at the bench shape: batch
32 x 120 x 160 logits up-sampled x4 to 480 x 640.

Pairs (forward with the loss, no stored probabilities, + backward): dice, dice_square, bootstrapped (keep_fraction 0.25), each plain
and _void on the SAME inputs; the training metric from the logits, plain and _void; the evaluation pass over stored probabilities and
uint8 class indices: Jaccard alone, Jaccard + confusion, Jaccard over the labelled pixels + confusion.  The labels carry a void frame
(the outer eighth on every side, 44 % of the pixels: a zoom-out's padding with fill_class = 255), so the void paths do their work; the
plain twins read the same bytes and compute the other answer.

Method: seeded inputs (logits normal(0, 2), uniform classes); 20 warm-up calls of each subject; then `repeats` rounds, in each round
every subject once in turn (twins next to each other), a subject's window = `calls` back-to-back calls between two HIP events on the
context's stream; time per call = window / calls.  Reported: median, min, max over the rounds.  The expectation checked at the end:
a void variant costs no more than its twin's median plus the twin's own max - min spread; the fused evaluation pass costs well under
two Jaccard passes.
usage: python scripts/mask_void_time.py [batch] [h] [w] [calls] [repeats] [--out FILE] [--commit TEXT]"""
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
ho, wo = h * f, w * f
hw = ho * wo
ctx = H.Context(0)
device = ctx.device_name()
logits = ctx.array(rng.normal(0, 2, (n, h, w, 4)).astype(np.float32))
y, prob, index = ctx.empty((n, ho, wo, 4)), ctx.empty((n, ho, wo, 4)), ctx.empty((n, ho, wo), np.uint8)
frame = np.ones((ho, wo), bool)
frame[ho // 8:ho - ho // 8, wo // 8:wo - wo // 8] = False
for b in range(n):          # one image at a time: 39 MB of one-hot rows per image on the host
    cls = rng.integers(0, 4, (ho, wo)).astype(np.uint8)
    cls[frame] = 255
    rows = np.eye(4, dtype=np.float32)[np.minimum(cls, 3)]
    rows[frame] = 0.0
    ctx.borrow(y.ptr + b * rows.nbytes, rows.shape, np.float32, owner=y).upload(rows)
    ctx.borrow(index.ptr + b * cls.nbytes, cls.shape, np.uint8, owner=index).upload(cls)
cw = (C.c_float * 4)(0.05, 0.575, 0.135, 0.24)
ctx.call("ssdseg_mask_head_fwd", logits, n, h, w, 4, f, f, None, None, prob, None)
loss, g, coef, metric = ctx.empty(n), ctx.empty((n, h, w, 4)), ctx.empty((n, 8)), ctx.empty(n)
pixel_loss, thresh, keep_dev, kept = ctx.empty((n, hw)), ctx.empty(n), ctx.empty(n, np.int32), ctx.empty(n, np.int32)
iou, confusion, void_px = ctx.empty((n, 4)), ctx.empty((n, 4, 4), np.int32), ctx.empty(n, np.int32)
scale = 1.0 / n
keep = LS.bootstrap_keep(fraction, hw)
head = (logits, n, h, w, 4, f, f)


def dice_pair(suffix, squared):
    def run():
        ctx.call("ssdseg_mask_head_fwd_dice" + suffix, *head, y, cw, squared, None, loss, coef)
        ctx.call("ssdseg_mask_head_bwd_dice" + suffix, *head, y, coef, squared, scale, g)
    return run


def bootstrap_pair():
    ctx.call("ssdseg_mask_head_fwd_bootstrap", *head, y, cw, keep, None, pixel_loss, thresh, kept, loss)
    ctx.call("ssdseg_mask_head_bwd_bootstrap", *head, y, cw, pixel_loss, thresh, scale, g)


def bootstrap_void_pair():
    ctx.call("ssdseg_mask_head_fwd_bootstrap_void", *head, y, cw, fraction, None, pixel_loss, thresh, keep_dev, kept, loss)
    ctx.call("ssdseg_mask_head_bwd_bootstrap_void", *head, y, cw, pixel_loss, thresh, scale, g)


subjects = {
    "dice pair": dice_pair("", 0), "dice pair, void": dice_pair("_void", 0),
    "dice_square pair": dice_pair("", 1), "dice_square pair, void": dice_pair("_void", 1),
    "bootstrapped pair": bootstrap_pair, "bootstrapped pair, void": bootstrap_void_pair,
    "metric from logits": lambda: ctx.call("ssdseg_metric_mask_iou", *head, 1, y, cw, metric),
    "metric from logits, void": lambda: ctx.call("ssdseg_metric_mask_iou_void", *head, 1, y, cw, metric),
    "eval Jaccard": lambda: ctx.call("ssdseg_eval_mask_jaccard", prob, index, n, hw, 4, iou),
    "eval scores: Jaccard + confusion": lambda: ctx.call("ssdseg_eval_mask_scores", prob, index, n, hw, 4, 0, iou, confusion, void_px),
    "eval scores: void Jaccard + confusion": lambda: ctx.call("ssdseg_eval_mask_scores", prob, index, n, hw, 4, 1, iou, confusion, void_px),
}
twins = [("dice pair", "dice pair, void"), ("dice_square pair", "dice_square pair, void"), ("bootstrapped pair", "bootstrapped pair, void"),
         ("metric from logits", "metric from logits, void")]

for fn in subjects.values():
    for _ in range(20):
        fn()
ctx.sync()
kept_host, keep_host, void_host = kept.download(), keep_dev.download(), void_px.download()

start, stop = ctx.event(), ctx.event()
windows = {name: [] for name in subjects}
for _ in range(repeats):
    for name, fn in subjects.items():
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        ctx.sync()
        windows[name].append(start.elapsed_ms(stop) / calls * 1e3)

lines = [f"Void-pixel variants of the mask losses and metric, and the fused evaluation pass, at {n} x {h} x {w} logits x{f} -> {ho} x {wo}, fp32, one GPU.",
         f"Command: python scripts/mask_void_time.py {n} {h} {w} {calls} {repeats}",
         f"commit: {commit}",
         f"device: {device}",
         f"labels: a void frame of {int(frame.sum())} of {hw} pixels per image ({100.0 * frame.mean():.0f} %); bootstrapped keep_fraction {fraction}: plain keep = {keep},",
         f"        void keep = {int(keep_host.min())} ... {int(keep_host.max())}, kept {int(kept_host.min())} ... {int(kept_host.max())}; void pixels per image by the evaluation pass: {int(void_host.min())} ... {int(void_host.max())}",
         f"{repeats} rounds, every subject once per round in turn; a window = {calls} back-to-back calls between two HIP events; microseconds per call",
         ""]
stats = {}
for name, win in windows.items():
    win = np.asarray(win)
    stats[name] = (float(np.median(win)), float(win.min()), float(win.max()))
    lines.append(f"{name:40s}: median {stats[name][0]:9.2f} us   min {stats[name][1]:9.2f}   max {stats[name][2]:9.2f}")
lines.append("")
for plain, void in twins:
    (pm, pmin, pmax), (vm, _, _) = stats[plain], stats[void]
    verdict = "within" if vm <= pm + (pmax - pmin) else "ABOVE"
    lines.append(f"{void:40s}: {vm - pm:+9.2f} us against its twin ({vm / pm:.3f}x); the twin's max - min spread is {pmax - pmin:.2f} us: {verdict} it")
jac = stats["eval Jaccard"][0]
for name in ("eval scores: Jaccard + confusion", "eval scores: void Jaccard + confusion"):
    lines.append(f"{name:40s}: {stats[name][0] / jac:.3f} Jaccard passes ({stats[name][0] - jac:+.2f} us); {n * hw * 17 / stats[name][0] / 1e3:.0f} GB/s of the {n * hw * 17 / 1e6:.0f} MB read")
text = "\n".join(lines) + "\n"
print(text, end="")
if "--out" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as fh:
        fh.write(text)
