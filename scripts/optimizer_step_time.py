#!/usr/bin/env python3
"""What one optimizer update costs at the full model's trainable count (MobileNetV2 + DeepLabV3+ + SSDLite at 480 x 640), with the
weight-decay run table that model produces (decay on `kernel` / `pointwise_kernel`, adjacent equal runs merged).
Yardstick: `ssdseg_adam_step` (28 B per element; the parent commit's code), measured in the same run.  Against it:
`ssdseg_sgd_step` with momentum 0.9 and the table (20 B per element), `ssdseg_adamw_step` with the table (28 B per element plus
the table), and for reference plain `ssdseg_sgd_step` without a table (12 B per element) and Nesterov with the table.

Method: seeded parameters, gradients and state; 20 warm-up calls of each entry; then `repeats` windows per entry, the entries
alternating, each window `calls` back-to-back calls between two HIP events on the context's stream; per-call time =
window / calls.  Reported: median, minimum, maximum and the quartiles of the windows of each entry, the achieved bandwidth at the
median, the two acceptance comparisons of the optimizer pull request (SGD with momentum no slower than Adam at the medians;
AdamW within Adam's median plus Adam's own max - min), and -- with --step-ms, the time of one `bench.py` training step measured
in the same sitting -- each update as a share of the step.
usage: python scripts/optimizer_step_time.py [calls] [repeats] [--out FILE] [--commit TEXT] [--step-ms MS]"""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
import bench
from ssdseglib import _hip as H
from ssdseglib import optimizers as Opt

args = sys.argv[1:]
opts = {}
for flag in ("--out", "--commit", "--step-ms"):
    if flag in args:
        i = args.index(flag)
        opts[flag] = args[i + 1]
        del args[i:i + 2]
calls = int(args[0]) if len(args) > 0 else 20
repeats = int(args[1]) if len(args) > 1 else 50
commit = opts.get("--commit")
if commit is None:
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        commit = "unknown (not a git checkout)"

_, builder = bench.build_models(seed=1993)
model = builder.get_model_for_training('deeplabv3plus', 'ssdlite', segmentation_dilation_rates=(3, 6, 12))
decay = Opt.SGD(momentum=0.9, weight_decay=5e-4)
ends, lams = Opt.model_decay_runs(model, decay)
count = int(ends[-1])
decayed = int((Opt.expand_runs(ends, lams, count) != 0).sum())

rng = np.random.default_rng(1993)
ctx = H.Context(0)
device = ctx.device_name()
g = ctx.array(rng.normal(0, 1e-2, count).astype(np.float32))
d_ends, d_lams, nruns = ctx.array(ends), ctx.array(lams), int(ends.size)
n = C.c_size_t(count)


def state():
    """a parameter bucket and two state buckets of an entry's own"""
    return (ctx.array(rng.normal(0, 0.1, count).astype(np.float32)), ctx.array(rng.normal(0, 1e-3, count).astype(np.float32)),
            ctx.array(rng.uniform(0, 1e-4, count).astype(np.float32)))


ADAM, SGDM, ADAMW, PLAIN, NEST = "adam (yardstick)", "sgd momentum + table", "adamw + table", "sgd plain, no table", "sgd nesterov + table"
bufs = {name: state() for name in (ADAM, SGDM, ADAMW, PLAIN, NEST)}
hyper = (1e-4, 0.9, 0.999, 1e-7, 1000, 1.0)


def sgd(name, momentum, nesterov, table):
    p, v, _ = bufs[name]
    return lambda: ctx.call("ssdseg_sgd_step", p, g, v if momentum else None, n, 1e-3, momentum, nesterov, 1.0, *table)


entries = {
    ADAM: lambda: ctx.call("ssdseg_adam_step", bufs[ADAM][0], g, bufs[ADAM][1], bufs[ADAM][2], n, *hyper),
    SGDM: sgd(SGDM, 0.9, 0, (d_ends, d_lams, nruns)),
    ADAMW: lambda: ctx.call("ssdseg_adamw_step", bufs[ADAMW][0], g, bufs[ADAMW][1], bufs[ADAMW][2], n, *hyper, d_ends, d_lams, nruns),
    PLAIN: sgd(PLAIN, 0.0, 0, (None, None, 0)),
    NEST: sgd(NEST, 0.9, 1, (d_ends, d_lams, nruns)),
}
BYTES = {ADAM: 28, SGDM: 20, ADAMW: 28, PLAIN: 12, NEST: 20}

for fn in entries.values():
    for _ in range(20):
        fn()
ctx.sync()

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

lines = [f"Optimizer updates over one flat bucket of {count} fp32 parameters (the full model's trainable count), one GPU.",
         f"Run table of that model for decay on kernel / pointwise_kernel: {nruns} runs, {decayed} elements decay "
         f"({int((ends[:-1] % 4 != 0).sum())} boundaries not on a multiple of 4).",
         f"Command: python scripts/optimizer_step_time.py {calls} {repeats}" + (f" --step-ms {opts['--step-ms']}" if "--step-ms" in opts else ""),
         f"commit: {commit}",
         f"device: {device}",
         f"{repeats} windows per entry, the entries alternating; a window = {calls} back-to-back calls between two HIP events; microseconds per call",
         ""]
stats = {}
for name, w in windows.items():
    w = np.asarray(w)
    q1, med, q3 = np.percentile(w, [25, 50, 75])
    stats[name] = (med, w.min(), w.max(), q1, q3)
    lines.append(f"{name:22s}: median {med:8.2f} us   min {w.min():8.2f}   max {w.max():8.2f}   quartiles {q1:8.2f} / {q3:8.2f}   "
                 f"{BYTES[name]} B/element -> {BYTES[name] * count / med / 1e6:6.2f} TB/s")
yard = stats[ADAM]
spread = yard[2] - yard[1]
lines += ["",
          f"run-to-run spread of the yardstick: interquartile range {yard[4] - yard[3]:.2f} us; full range (max - min) {spread:.2f} us",
          f"sgd momentum + table - yardstick, medians: {stats[SGDM][0] - yard[0]:+.2f} us ({100 * (stats[SGDM][0] / yard[0] - 1):+.1f} %)   "
          f"acceptance (<= yardstick median): {'met' if stats[SGDM][0] <= yard[0] else 'MISSED'}",
          f"adamw + table        - yardstick, medians: {stats[ADAMW][0] - yard[0]:+.2f} us ({100 * (stats[ADAMW][0] / yard[0] - 1):+.1f} %)   "
          f"acceptance (<= yardstick median + its full range = {yard[0] + spread:.2f} us): {'met' if stats[ADAMW][0] <= yard[0] + spread else 'MISSED'}"]
if "--step-ms" in opts:
    step_ms = float(opts["--step-ms"])
    lines.append(f"share of one bench.py training step ({step_ms:.2f} ms, measured in the same sitting): "
                 + ", ".join(f"{name} {100 * stats[name][0] / (step_ms * 1e3):.3f} %" for name in entries))
text = "\n".join(lines) + "\n"
print(text, end="")
if "--out" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as f:
        f.write(text)
