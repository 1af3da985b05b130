#!/usr/bin/env python3
"""What gradient clipping and the EMA of the weights cost at the full model's trainable count (MobileNetV2 + DeepLabV3+ + SSDLite at
480 x 640), with the weight-decay run table that model produces (decay on `kernel` / `pointwise_kernel`, adjacent equal runs
merged).  Yardstick: `ssdseg_sgd_step` with momentum 0.9 and the table (20 B per element; code from before clipping), measured in
the same run.  Against it: `ssdseg_grad_norm` (one 4 B per element read), `ssdseg_sgd_step_clipped` (the yardstick's twin: the
factor from the norm entry's buffer), `ssdseg_adamw_step_clipped` with the table next to its twin `ssdseg_adamw_step` (28 B per
element), and `ssdseg_ema_update` (12 B per element).

Method, as scripts/optimizer_step_time.py: seeded parameters, gradients and state; 20 warm-up calls of each entry; then `repeats`
windows per entry, the entries alternating, each window `calls` back-to-back calls between two HIP events on the context's stream;
per-call time = window / calls.  Reported: median, minimum, maximum and the quartiles of the windows of each entry, the achieved
bandwidth at the median, each clipped step against its unclipped twin at the medians with the twin's own max - min as the spread,
the norm entry against its 4 B per element floor at the bandwidth the plain 12 B per element update reaches in this run, and -- with
--step-ms, the time of one `bench.py` training step measured in the same sitting -- clipped step + norm + EMA as a share of the step.
usage: python scripts/optimizer_clip_time.py [calls] [repeats] [--out FILE] [--commit TEXT] [--step-ms MS]"""
import ctypes as C
import math
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
ends, lams = Opt.model_decay_runs(model, Opt.SGD(momentum=0.9, weight_decay=5e-4))
count = int(ends[-1])

rng = np.random.default_rng(1993)
ctx = H.Context(0)
device = ctx.device_name()
grad = rng.normal(0, 1e-2, count).astype(np.float32)
g = ctx.array(grad)
d_ends, d_lams, nruns = ctx.array(ends), ctx.array(lams), int(ends.size)
table = (d_ends, d_lams, nruns)
n = C.c_size_t(count)
nparts = ctx.lib.ssdseg_grad_norm_parts(count)
partials, clip = ctx.empty(nparts, np.float64), ctx.zeros(2)
CLIP_NORM = 1.0           # below the seeded bucket's norm (about 20): the factor the clipped steps read is a real one
factor = clip.view(1, (1,))


def state():
    """a parameter bucket and two state buckets of an entry's own"""
    return (ctx.array(rng.normal(0, 0.1, count).astype(np.float32)), ctx.array(rng.normal(0, 1e-3, count).astype(np.float32)),
            ctx.array(rng.uniform(0, 1e-4, count).astype(np.float32)))


SGDM, SGDC, ADAMW, ADAMWC, PLAIN, NORM, EMA = ("sgd momentum + table (yardstick)", "sgd momentum clipped", "adamw + table", "adamw clipped",
                                              "sgd plain, no table", "grad norm", "ema update")
bufs = {name: state() for name in (SGDM, SGDC, ADAMW, ADAMWC, PLAIN, EMA)}
hyper = (1e-4, 0.9, 0.999, 1e-7, 1000, 1.0)


def sgd(name, suffix="", extra=()):
    p, v, _ = bufs[name]
    return lambda: ctx.call("ssdseg_sgd_step" + suffix, p, g, v, n, 1e-3, 0.9, 0, 1.0, *table, *extra)


def adamw(name, suffix="", extra=()):
    p, m, v = bufs[name]
    return lambda: ctx.call("ssdseg_adamw_step" + suffix, p, g, m, v, n, *hyper, *table, *extra)


entries = {
    SGDM: sgd(SGDM),
    SGDC: sgd(SGDC, "_clipped", (factor, math.inf)),
    ADAMW: adamw(ADAMW),
    ADAMWC: adamw(ADAMWC, "_clipped", (factor, math.inf)),
    PLAIN: lambda: ctx.call("ssdseg_sgd_step", bufs[PLAIN][0], g, None, n, 1e-3, 0.0, 0, 1.0, None, None, 0),
    NORM: lambda: ctx.call("ssdseg_grad_norm", g, n, 1.0, CLIP_NORM, partials, clip),
    EMA: lambda: ctx.call("ssdseg_ema_update", bufs[EMA][1], bufs[EMA][0], n, 0.99),
}
BYTES = {SGDM: 20, SGDC: 20, ADAMW: 28, ADAMWC: 28, PLAIN: 12, NORM: 4, EMA: 12}

entries[NORM]()
norm, fac = clip.download()
want_norm, want_fac = Opt._clip_reference(grad, 1.0, CLIP_NORM)
assert abs(norm - want_norm) <= 2e-7 * want_norm and abs(fac - want_fac) <= 2e-7 * want_fac < 1, (norm, fac, want_norm, want_fac)

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

lines = [f"Gradient clipping and EMA over one flat bucket of {count} fp32 parameters (the full model's trainable count), one GPU.",
         f"Run table of that model for decay on kernel / pointwise_kernel: {nruns} runs.  Norm entry: {nparts} fp64 partials; the seeded bucket's "
         f"norm {norm:.6g}, clip_norm {CLIP_NORM:g}, factor {fac:.6g} (the clipped steps read it from device memory; clip_value +inf).",
         f"Command: python scripts/optimizer_clip_time.py {calls} {repeats}" + (f" --step-ms {opts['--step-ms']}" if "--step-ms" in opts else ""),
         f"commit: {commit}",
         f"device: {device}",
         f"{repeats} windows per entry, the entries alternating; a window = {calls} back-to-back calls between two HIP events; microseconds per call",
         ""]
stats = {}
for name, w in windows.items():
    w = np.asarray(w)
    q1, med, q3 = np.percentile(w, [25, 50, 75])
    stats[name] = (med, w.min(), w.max(), q1, q3)
    lines.append(f"{name:32s}: median {med:8.2f} us   min {w.min():8.2f}   max {w.max():8.2f}   quartiles {q1:8.2f} / {q3:8.2f}   "
                 f"{BYTES[name]:2d} B/element -> {BYTES[name] * count / med / 1e6:6.2f} TB/s")
lines.append("")
for twin, clipped in ((SGDM, SGDC), (ADAMW, ADAMWC)):
    t, c = stats[twin], stats[clipped]
    lines.append(f"{clipped} - {twin}, medians: {c[0] - t[0]:+.2f} us ({100 * (c[0] / t[0] - 1):+.1f} %); "
                 f"the twin's own spread (max - min) {t[2] - t[1]:.2f} us, interquartile range {t[4] - t[3]:.2f} us")
floor = 4 * count / (BYTES[PLAIN] * count / stats[PLAIN][0])
lines.append(f"grad norm against its 4 B/element floor: {stats[NORM][0]:.2f} us for two launches; 4 B/element at the bandwidth of the plain 12 B/element "
             f"update of this run would be {floor:.2f} us ({stats[NORM][0] / floor:.2f} x)")
total = stats[SGDC][0] + stats[NORM][0] + stats[EMA][0]
lines.append(f"clipped sgd step + norm + ema update: {total:.2f} us against {stats[SGDM][0]:.2f} us for the unclipped step alone")
if "--step-ms" in opts:
    step_ms = float(opts["--step-ms"])
    lines.append(f"share of one bench.py training step ({step_ms:.2f} ms, measured in the same sitting): clipped sgd step + norm + ema update "
                 f"{100 * total / (step_ms * 1e3):.3f} %; " + ", ".join(f"{name} {100 * stats[name][0] / (step_ms * 1e3):.3f} %" for name in (SGDC, NORM, EMA)))
text = "\n".join(lines) + "\n"
print(text, end="")
if "--out" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
    with open(opts["--out"], "w") as f:
        f.write(text)
