"""Optimizer descriptions for `model.compile`, learning-rate schedules, and the optimizer's part of a checkpoint.

`Adam` stands in for `tf.keras.optimizers.Adam(learning_rate=1e-4)` of NB03#cell14 (Keras 2.13 defaults: beta_1 0.9, beta_2 0.999,
epsilon 1e-7); `SGD` for `tf.keras.optimizers.SGD`, the optimizer of the recipes the two heads come from (SSD: momentum 0.9, L2
decay 5e-4, stepped rate; DeepLabV3+: momentum and the "poly" rate; MobileNetV2: decay on the convolution kernels only).  Both
take Keras 2.13's decoupled `weight_decay`, applied to the weights named in `weight_decay_names`.  The updates themselves are
the fused HIP kernels ssdseg_adam_step / ssdseg_adamw_step / ssdseg_sgd_step over the flat parameter bucket (include/ssdseg.h);
`_sgd_reference` and `_adamw_reference` below are their specification, as `_augment_spec._mosaic_resample` is the mosaic kernel's.
Both also take Keras' `global_clipnorm` / `clipvalue` and `use_ema` / `ema_momentum` / `ema_overwrite_frequency`: the clip factor is
produced and consumed on the device (ssdseg_grad_norm, then ssdseg_sgd_step_clipped / ssdseg_adamw_step_clipped), the average is
a pass after the step (ssdseg_ema_update); `_clip_reference` and `_ema_reference` are their specifications, and
`averaged_weights` / `finalize_variable_values` put the average where predict, evaluate and Model.save see it.
Everything here works from the graph and NumPy.  The state on the device and the step itself are `_optim.OptimState`; the checkpoint
and the averaged-weights functions reach it through the model (`model._optim`, set with the model's first engine), so this module
imports neither that module nor the engine's.

A learning rate is a float or a schedule: a callable `step -> float`, evaluated on the host in float64 with `step` = the number
of updates already applied (0 for the first), and rounded once to float32 where it is handed to the kernel.
"""
import math

import numpy as np

DECAY_NAMES = ("kernel", "pointwise_kernel")      # not depthwise_kernel, bias, gamma, beta: the MobileNetV2 recipe


# ===================================================================================================== schedules
class PiecewiseConstantDecay:
    """Keras 2.13 `PiecewiseConstantDecay(boundaries, values)`, len(values) == len(boundaries) + 1:
        lr(step) = values[0]      for step <= boundaries[0]
                   values[i]      for boundaries[i-1] < step <= boundaries[i]
                   values[-1]     for step > boundaries[-1]"""

    def __init__(self, boundaries, values):
        self.boundaries, self.values = [float(b) for b in boundaries], [float(v) for v in values]
        if len(self.values) != len(self.boundaries) + 1:
            raise ValueError("PiecewiseConstantDecay: len(values) must be len(boundaries) + 1")
        if any(b1 <= b0 for b0, b1 in zip(self.boundaries, self.boundaries[1:])):
            raise ValueError("PiecewiseConstantDecay: boundaries must ascend")

    def __call__(self, step) -> float:
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]


class PolynomialDecay:
    """Keras 2.13 `PolynomialDecay` without `cycle` (power 1, end 0: the "poly" rate of DeepLab at power 0.9):
        s = min(step, decay_steps)
        lr(step) = (initial_learning_rate - end_learning_rate) * (1 - s / decay_steps) ** power + end_learning_rate"""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=1e-4, power=1.0):
        self.initial_learning_rate, self.decay_steps = float(initial_learning_rate), float(decay_steps)
        self.end_learning_rate, self.power = float(end_learning_rate), float(power)
        if self.decay_steps <= 0:
            raise ValueError("PolynomialDecay: decay_steps must be positive")

    def __call__(self, step) -> float:
        s = min(float(step), self.decay_steps)
        return (self.initial_learning_rate - self.end_learning_rate) * (1.0 - s / self.decay_steps) ** self.power + self.end_learning_rate


class CosineDecay:
    """Keras 2.13 `CosineDecay`.  With cosine(s, from) = from * ((1 - alpha) * 0.5 * (1 + cos(pi * s / decay_steps)) + alpha):
        warmup_target is None:  lr(step) = cosine(min(step, decay_steps), initial_learning_rate)
        otherwise, s = min(step, warmup_steps + decay_steps):
            s <  warmup_steps:  lr = initial_learning_rate + (warmup_target - initial_learning_rate) * s / warmup_steps
            s >= warmup_steps:  lr = cosine(s - warmup_steps, warmup_target)"""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, warmup_target=None, warmup_steps=0):
        self.initial_learning_rate, self.decay_steps, self.alpha = float(initial_learning_rate), float(decay_steps), float(alpha)
        self.warmup_target = None if warmup_target is None else float(warmup_target)
        self.warmup_steps = float(warmup_steps)
        if self.decay_steps <= 0:
            raise ValueError("CosineDecay: decay_steps must be positive")

    def _cosine(self, s, start):
        return start * ((1.0 - self.alpha) * 0.5 * (1.0 + math.cos(math.pi * s / self.decay_steps)) + self.alpha)

    def __call__(self, step) -> float:
        if self.warmup_target is None:
            return self._cosine(min(float(step), self.decay_steps), self.initial_learning_rate)
        s = min(float(step), self.warmup_steps + self.decay_steps)
        if s < self.warmup_steps:
            return self.initial_learning_rate + (self.warmup_target - self.initial_learning_rate) * s / self.warmup_steps
        return self._cosine(s - self.warmup_steps, self.warmup_target)


def is_schedule(learning_rate) -> bool:
    return callable(learning_rate)


def rate_at(learning_rate, step: int) -> float:
    """the rate of the update that follows `step` applied ones: the float itself, or the schedule's float64 value"""
    return float(learning_rate(int(step))) if callable(learning_rate) else learning_rate


# ===================================================================================================== optimizers
class _Optimizer:
    kind = ""
    slots = ()          # the per-parameter state arrays of this optimizer, as a checkpoint names them

    def _common(self, learning_rate, weight_decay, weight_decay_names):
        self.learning_rate = learning_rate if callable(learning_rate) else float(learning_rate)
        self.weight_decay = float(weight_decay)
        self.weight_decay_names = tuple(weight_decay_names)
        if self.weight_decay < 0:
            raise ValueError("weight_decay must not be negative")

    def _clip_and_ema(self, global_clipnorm, clipvalue, use_ema, ema_momentum, ema_overwrite_frequency, clipnorm):
        """the base-class arguments of Keras 2.13's optimizers that act on the gradient before, and on the weights after, the update:
            global_clipnorm : g' = g * min(1, global_clipnorm / ||g||) over ALL gradients (tf.clip_by_global_norm)
            clipvalue       : g' = clip(g, -clipvalue, clipvalue) elementwise (tf.clip_by_value)
            use_ema         : ema = ema_momentum * ema + (1 - ema_momentum) * p after every update, ema = p before the first;
                              with ema_overwrite_frequency = k the weights take the average after every k-th update
        The gradient is the one after `grad_scale` (the mean over the ranks); the clip comes before the decay and the update."""
        if clipnorm is not None:
            raise NotImplementedError("clipnorm (the per-variable norm) is not implemented: use global_clipnorm, the norm over all gradients")
        self.global_clipnorm = None if global_clipnorm is None else float(global_clipnorm)
        self.clipvalue = None if clipvalue is None else float(clipvalue)
        for name in ("global_clipnorm", "clipvalue"):
            v = getattr(self, name)
            if v is not None and not v > 0:
                raise ValueError(f"{name} must be positive")
        if self.global_clipnorm is not None and self.clipvalue is not None:
            raise ValueError("at most one of global_clipnorm and clipvalue may be set")
        self.use_ema, self.ema_momentum = bool(use_ema), float(ema_momentum)
        if not 0.0 <= self.ema_momentum <= 1.0:
            raise ValueError("ema_momentum must be in [0, 1]")
        if ema_overwrite_frequency is not None and (isinstance(ema_overwrite_frequency, bool) or not isinstance(ema_overwrite_frequency, (int, np.integer))
                                                    or ema_overwrite_frequency < 1):
            raise ValueError("ema_overwrite_frequency must be a positive int or None")
        self.ema_overwrite_frequency = None if ema_overwrite_frequency is None else int(ema_overwrite_frequency)


class Adam(_Optimizer):
    """Keras 2.13 Adam; with weight_decay > 0, p -= learning_rate * weight_decay * p on the `weight_decay_names` weights first
    (the rate itself, not the bias-corrected one).  Clipping and EMA: `_Optimizer._clip_and_ema`."""
    kind, slots = "adam", ("m", "v")

    def __init__(self, learning_rate=1e-3, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7, weight_decay: float = 0.0,
                 weight_decay_names=DECAY_NAMES, global_clipnorm=None, clipvalue=None, use_ema: bool = False, ema_momentum: float = 0.99,
                 ema_overwrite_frequency=None, clipnorm=None):
        self._common(learning_rate, weight_decay, weight_decay_names)
        self._clip_and_ema(global_clipnorm, clipvalue, use_ema, ema_momentum, ema_overwrite_frequency, clipnorm)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)


class SGD(_Optimizer):
    """Keras 2.13 SGD: v = momentum v - lr g, p += v (Nesterov: p += momentum v - lr g); momentum 0: p -= lr g.  weight_decay as Adam's.
    Clipping and EMA: `_Optimizer._clip_and_ema`."""
    kind = "sgd"

    def __init__(self, learning_rate=0.01, momentum: float = 0.0, nesterov: bool = False, weight_decay: float = 0.0,
                 weight_decay_names=DECAY_NAMES, global_clipnorm=None, clipvalue=None, use_ema: bool = False, ema_momentum: float = 0.99,
                 ema_overwrite_frequency=None, clipnorm=None):
        self._common(learning_rate, weight_decay, weight_decay_names)
        self._clip_and_ema(global_clipnorm, clipvalue, use_ema, ema_momentum, ema_overwrite_frequency, clipnorm)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError("momentum must be in [0, 1)")

    @property
    def slots(self):
        return ("velocity",) if self.momentum > 0 else ()


# ===================================================================================================== the run table
def bucket_entries(model):
    """[(layer, weight name, offset, size)] of the trainable weights in the order of the engine's flat parameter bucket (layer
    order, then the layer's own weight order) -- from the graph alone, no device"""
    out, off = [], 0
    for l in model.layers:
        for wname, arr in l.weights.items():
            if wname in l.trainable_names:
                out.append((l, wname, off, int(arr.size)))
                off += int(arr.size)
    return out


def decay_runs(entries, weight_decay: float, names):
    """the kernels' run table (include/ssdseg.h) for `entries` = (weight name, offset, size) in bucket order -> (run_end int64,
    run_decay float32): lambda = weight_decay for the weights in `names`, 0 for the others, adjacent equal-lambda runs merged.
    No decay at all is the empty table."""
    ends, lams = [], []
    if weight_decay != 0.0:
        at = 0
        for wname, off, size in entries:
            assert off == at, "entries are not the contiguous bucket"
            at = off + size
            if size == 0:
                continue
            lam = weight_decay if wname in names else 0.0
            if lams and lams[-1] == lam:
                ends[-1] = at
            else:
                ends.append(at)
                lams.append(lam)
    return np.asarray(ends, np.int64), np.asarray(lams, np.float32)


def model_decay_runs(model, optimizer):
    """the run table `optimizer` gives `model`, from the graph alone"""
    return decay_runs([(w, off, size) for _, w, off, size in bucket_entries(model)], optimizer.weight_decay, optimizer.weight_decay_names)


def expand_runs(run_end, run_decay, count: int, dtype=np.float64):
    """the per-element lambda the kernels derive from a run table: run r covers [run_end[r-1], run_end[r]); 0 from the last end on"""
    lam = np.zeros(count, dtype)
    at = 0
    for end, l in zip(np.asarray(run_end, np.int64).tolist(), np.asarray(run_decay).tolist()):
        end = min(end, count)
        if end > at:
            lam[at:end] = l
            at = end
    return lam


# ===================================================================================================== specifications
def _decayed(p, lr, run_end, run_decay):
    if run_end is None or len(run_end) == 0:
        return p
    lam = expand_runs(run_end, run_decay, p.size, p.dtype).reshape(p.shape)
    return p - (p.dtype.type(lr) * lam) * p


def _clip_reference(g, grad_scale=1.0, global_clipnorm=None):
    """ssdseg_grad_norm in float64 -> (norm, factor): norm = |grad_scale| sqrt(sum g^2) over ALL of `g`, factor = global_clipnorm / norm
    where the norm exceeds a positive, finite global_clipnorm, and 1 otherwise (also for a zero or a NaN norm)"""
    g = np.asarray(g, np.float64).reshape(-1)
    norm = abs(float(grad_scale)) * math.sqrt(float(np.dot(g, g)))
    c = 0.0 if global_clipnorm is None else float(global_clipnorm)
    return norm, (c / norm if c > 0 and math.isfinite(c) and norm > c else 1.0)


def _clipped(gk, clip_scale, clip_value):
    """g' = clampv(gk * s, c) of the *_clipped entries, in the dtype of `gk`; NaN passes through; the defaults change nothing"""
    t = gk.dtype.type
    if clip_scale == 1.0 and clip_value == math.inf:
        return gk
    x, c = gk * t(clip_scale), t(clip_value)
    return np.where(x < -c, -c, np.where(x > c, c, x))


def _ema_reference(ema, p, momentum):
    """ssdseg_ema_update in NumPy, in the dtype of `ema`: ema + (p - ema) (1 - momentum), 1 - momentum formed once in float32"""
    t = ema.dtype.type
    return ema + (p.astype(ema.dtype) - ema) * t(np.float32(1.0) - np.float32(momentum))


def _sgd_reference(p, g, v, lr, momentum=0.0, nesterov=False, grad_scale=1.0, run_end=None, run_decay=None, clip_scale=1.0, clip_value=math.inf):
    """ssdseg_sgd_step in NumPy, in the dtype of `p` -> (p, v); v may be None when momentum == 0 and comes back as it went in.
    With clip_scale / clip_value: ssdseg_sgd_step_clipped."""
    t = p.dtype.type
    gk = _clipped(g.astype(p.dtype) * t(grad_scale), clip_scale, clip_value)
    p1 = _decayed(p, lr, run_end, run_decay)
    if momentum == 0:
        return p1 - t(lr) * gk, v
    v = t(momentum) * v.astype(p.dtype) - t(lr) * gk
    return (p1 + (t(momentum) * v - t(lr) * gk) if nesterov else p1 + v), v


def _adamw_reference(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, grad_scale=1.0, run_end=None, run_decay=None, clip_scale=1.0,
                     clip_value=math.inf):
    """ssdseg_adamw_step in NumPy, in the dtype of `p` -> (p, m, v); `step` counts from 1, as the kernel's.
    With clip_scale / clip_value: ssdseg_adamw_step_clipped."""
    t = p.dtype.type
    gk = _clipped(g.astype(p.dtype) * t(grad_scale), clip_scale, clip_value)
    p1 = _decayed(p, lr, run_end, run_decay)
    m = m + (gk - m) * t(1.0 - b1)
    v = v + (gk * gk - v) * t(1.0 - b2)
    alpha = t(lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step))
    return p1 - alpha * m / (np.sqrt(v) + t(eps)), m, v


# ===================================================================================================== checkpoint
def state_slots(opt):
    """the optimizer's slots plus `ema`, the averaged weights, when it keeps them"""
    return tuple(opt.slots) + (("ema",) if opt.use_ema else ())


def _compiled_optimizer(model):
    comp = getattr(model, "_compiled", None)
    if not comp or comp.get("optimizer") is None:
        raise ValueError("the model has no compiled optimizer: call model.compile(optimizer=...) first")
    return comp["optimizer"]


def get_state(model):
    """-> (kind, step, {`<layer>/<weight>:<slot>`: array}) of the model's compiled optimizer: from the device once the model has
    trained, otherwise what `set_state` left for the first step, otherwise the initial state (step 0, zeros; `:ema`, which only an
    optimizer with use_ema has: the weights)"""
    opt = _compiled_optimizer(model)
    pending = model.__dict__.get("_optimizer_state")
    if pending is not None:
        return pending["kind"], pending["step"], {k: a.copy() for k, a in pending["arrays"].items()}
    state = getattr(model, "_optim", None)          # _optim.OptimState, once the model has an engine
    arrays = {}
    for slot in state_slots(opt):
        flat = state.download(slot) if state is not None else None
        for l, wname, off, size in bucket_entries(model):
            shape = l.weights[wname].shape
            initial = np.array(l.weights[wname], np.float32) if slot == "ema" else np.zeros(shape, np.float32)
            arrays[f"{l.name}/{wname}:{slot}"] = flat[off:off + size].reshape(shape).copy() if flat is not None else initial
    return opt.kind, int(state.step) if state is not None else 0, arrays


def set_state(model, kind: str, step: int, arrays) -> None:
    """hand the compiled optimizer its state; it takes effect at the next training step (the model need not have trained yet).
    Raises on a kind other than the compiled optimizer's, a missing key or a shape mismatch."""
    opt = _compiled_optimizer(model)
    if kind != opt.kind:
        raise ValueError(f"optimizer state of kind {kind!r} for a model compiled with {opt.kind!r}")
    kept = {}
    for l, wname, _, _ in bucket_entries(model):
        for slot in state_slots(opt):
            key = f"{l.name}/{wname}:{slot}"
            if key not in arrays:
                raise KeyError(f"optimizer state has no {key}")
            a = np.asarray(arrays[key], np.float32)
            if a.shape != l.weights[wname].shape:
                raise ValueError(f"optimizer state {key}: shape {a.shape} != {l.weights[wname].shape}")
            kept[key] = a.copy()
    model._optimizer_state = dict(kind=kind, step=int(step), arrays=kept)


def _npz(path) -> str:
    return path if str(path).endswith(".npz") else str(path) + ".npz"


def save_state(model, path) -> None:
    """the optimizer's part of a checkpoint, next to `Model.save`: one .npz with `step`, `kind` and the state arrays keyed
    `<layer>/<weight>:m`, `:v` (Adam) or `:velocity` (SGD with momentum), and `:ema` with use_ema -- names and shapes, not the
    bucket layout"""
    kind, step, arrays = get_state(model)
    np.savez(_npz(path), step=np.int64(step), kind=np.asarray(kind), **arrays)


def load_state(model, path) -> None:
    """`save_state`'s file into a compiled model (freshly built, or trained); with `Model.load_weights`, which carries the weights
    and the BatchNorm moving statistics, the continued run is bit-identical to the uninterrupted one"""
    data = np.load(_npz(path))
    for key in ("step", "kind"):
        if key not in data.files:
            raise KeyError(f"{path}: not an optimizer state file (no {key})")
    set_state(model, str(data["kind"]), int(data["step"]), {k: data[k] for k in data.files if k not in ("step", "kind")})


# ===================================================================================================== averaged weights
def _ema_state(model):
    """the optimizer state (_optim.OptimState) of a model whose optimizer keeps averaged weights, with what `set_state` left applied;
    None before the model's first engine: the average IS the weights then"""
    opt = _compiled_optimizer(model)
    if not opt.use_ema:
        raise ValueError("the compiled optimizer keeps no averaged weights: build it with use_ema=True")
    state = getattr(model, "_optim", None)
    if state is None:
        if model.__dict__.get("_optimizer_state") is not None:
            raise RuntimeError("the restored averaged weights reach the device with the model's first engine: call predict or train once")
        return None
    state.restore()
    return state


def finalize_variable_values(model) -> None:
    """Keras' `optimizer.finalize_variable_values`: the weights become the averaged weights, for good"""
    state = _ema_state(model)
    if state is not None:
        state.finalize()


class averaged_weights:
    """`with averaged_weights(model):` -- inside, the parameter bucket holds the EMA, so predict, evaluate_on_device and Model.save
    see the averaged weights; the raw weights wait in a backup bucket (allocated on first use) and are back bit for bit on exit,
    also when the block raises.  Copies, not a pointer swap: every view into the bucket is an address.  BatchNorm's moving
    statistics are not averaged.  A training step inside the block raises."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        state = _ema_state(self.model)
        self.state = state if state is not None and state.swap_in_average() else None      # None: no update yet, the weights are the average
        return self.model

    def __exit__(self, *exc):
        if self.state is not None:
            self.state.swap_out_average()
        return False
