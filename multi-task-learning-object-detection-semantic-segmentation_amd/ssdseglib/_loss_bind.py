"""What connects a compiled loss or metric to its launches: one variant class per loss family (its device state and its entry
points of include/ssdseg.h), one table from the `losses` callables to those variants, one from `metric_kind` to the metric launches,
and the bodies of `Engine.configure_losses` / `configure_metrics` / `compute_metrics`.  `MaskHeadOp` and `DetLossOp` delegate
to the variants bound here; nothing else knows a loss by name.

Adding a loss: the callable in `losses` (with a `loss_kind`), one variant class here, one row of `LOSSES`.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial

import numpy as np

from . import _hip as H
from . import losses as LS
from ._ops import DetLossOp, MaskHeadOp, Op


@dataclass
class LossBinding:
    """one compiled loss of one model output, bound to the fused loss op that computes it"""
    name: str                   # the output's (Keras) name
    op: Op                      # MaskHeadOp | DetLossOp
    kind: str                   # "mask" | "conf" | "loc"
    target: H.DeviceBuffer      # what the step reads as y_true
    loss: H.DeviceBuffer        # per-sample loss [batch]
    weight: float               # its share of the total `loss`

    def __iter__(self):         # unpacks as (name, op, kind)
        return iter((self.name, self.op, self.kind))


# ====================================================================================================== mask-loss variants
# `MaskHeadOp` keeps what they share (y_true, class_weights, loss, loss_scale); a variant owns what its forward leaves for its backward
def _head(op: MaskHeadOp):
    s = op.logits.store
    return s.buf, s.n, s.h, s.w, s.c, op.fy, op.fx, op.y_true


def _void_suffix(fn) -> str:
    """what `ignore_void` on a loss or metric callable adds to its entries' names"""
    return "_void" if getattr(fn, "ignore_void", False) else ""


class CrossEntropy:
    """losses.cross_entropy (reference losses.py:294-305)"""

    def __init__(self, fn, ctx, batch, pixels):
        self.kind = fn.loss_kind

    def fwd(self, op, prob):
        op.e.ctx.call("ssdseg_mask_head_fwd", *_head(op), op.class_weights, prob, op.loss)

    def bwd(self, op, g):
        op.e.ctx.call("ssdseg_mask_head_bwd", *_head(op), op.class_weights, op.loss_scale, g)


class Dice:
    """losses.dice / dice_square (reference losses.py:175-262); `ignore_void` on the callable selects the _void pair"""

    def __init__(self, fn, ctx, batch, pixels, squared=0):
        self.kind, self.squared = fn.loss_kind, squared
        self.void = _void_suffix(fn)
        self.coef = ctx.empty((batch, 8))           # per-image backward coefficients left by the forward

    def fwd(self, op, prob):
        op.e.ctx.call("ssdseg_mask_head_fwd_dice" + self.void, *_head(op), op.class_weights, self.squared, prob, op.loss, self.coef)

    def bwd(self, op, g):
        op.e.ctx.call("ssdseg_mask_head_bwd_dice" + self.void, *_head(op), self.coef, self.squared, op.loss_scale, g)


class Bootstrapped:
    """losses.bootstrapped_cross_entropy: pixels kept per image, and what the forward leaves for the backward -- every pixel's loss
    [n][H*W], the per-image threshold [n] -- and the per-image kept count [n]"""

    def __init__(self, fn, ctx, batch, pixels):
        self.kind, self.keep = fn.loss_kind, LS.bootstrap_keep(fn.keep_fraction, pixels)
        self.pixel_loss, self.thresh, self.kept = ctx.empty((batch, pixels)), ctx.empty(batch), ctx.empty(batch, np.int32)

    def fwd(self, op, prob):
        op.e.ctx.call("ssdseg_mask_head_fwd_bootstrap", *_head(op), op.class_weights, self.keep, prob, self.pixel_loss, self.thresh,
                      self.kept, op.loss)

    def bwd(self, op, g):
        op.e.ctx.call("ssdseg_mask_head_bwd_bootstrap", *_head(op), op.class_weights, self.pixel_loss, self.thresh, op.loss_scale, g)


class BootstrappedVoid(Bootstrapped):
    """bootstrapped_cross_entropy(..., ignore_void=True): `keep` is a device buffer [n], written by the forward from the labelled
    pixels of the batch the device sees (crop and mosaic happen there); no host synchronisation"""

    def __init__(self, fn, ctx, batch, pixels):
        self.kind, self.keep_fraction, self.keep = fn.loss_kind, float(fn.keep_fraction), ctx.empty(batch, np.int32)
        self.pixel_loss, self.thresh, self.kept = ctx.empty((batch, pixels)), ctx.empty(batch), ctx.empty(batch, np.int32)

    def fwd(self, op, prob):
        op.e.ctx.call("ssdseg_mask_head_fwd_bootstrap_void", *_head(op), op.class_weights, self.keep_fraction, prob, self.pixel_loss,
                      self.thresh, self.keep, self.kept, op.loss)

    def bwd(self, op, g):
        op.e.ctx.call("ssdseg_mask_head_bwd_bootstrap_void", *_head(op), op.class_weights, self.pixel_loss, self.thresh, op.loss_scale, g)


# ====================================================================================================== detection-loss variants
# two independent axes of `DetLossOp`: `conf_impl.fwd(op, ins, outs)` is the fused confidence entry, `loc_impl.fwd(op)` what runs behind it; a
# constructor (fn, output name, output Val) raises where the loss does not fit the output, and touches no device
class Mined:
    """losses.confidence_loss.  Equal weights take the single-scale entry, the step's bits from before the weights could differ; so
    does an IoU localization loss, whose own entry applies `w_loc`"""
    kind = "mined"

    def fwd(self, op, ins, outs):
        n = op.probs.n
        if op.w_conf == op.w_loc or not op.loc_impl.fused:
            op.e.ctx.call("ssdseg_det_loss", *ins, op.w_conf / n, *outs, None)
        else:
            op.e.ctx.call("ssdseg_det_loss_scaled", *ins, op.w_conf / n, op.w_loc / n, *outs, None)


class Focal:
    """losses.focal_confidence_loss(alpha, gamma)"""
    kind = "focal"

    def __init__(self, fn, name, v):
        if "logits" not in v.meta:
            raise ValueError(f"loss {fn.__name__} does not fit output {name}: it takes the class probabilities")
        self.alpha, self.gamma = LS.c4(fn.alpha), float(fn.gamma)

    def fwd(self, op, ins, outs):
        n = op.probs.n
        op.e.ctx.call("ssdseg_det_loss_focal", *ins, self.alpha, self.gamma, op.w_conf / n, op.w_loc / n, *outs)


class SmoothL1:
    """losses.localization_loss: fused into the confidence entry, nothing runs behind it"""
    fn, kind, fused = None, 0, True

    def fwd(self, op):
        pass


class IouLoc:
    """losses.iou_localization_loss(...): `fn` is that callable, `kind` its kind's number"""
    fused = False

    def __init__(self, fn, name, v):
        if not v.meta.get("head_concat") or "logits" in v.meta:
            raise ValueError(f"loss {fn.__name__} does not fit output {name}: it takes the box offsets")
        if fn.n_anchors != v.store.h * v.store.w:
            raise ValueError(f"loss {fn.__name__}: {fn.n_anchors} default boxes, output {name} has {v.store.h * v.store.w} anchors")
        self.fn, self.kind = fn, LS.IOU_KINDS[fn.kind]

    def fwd(self, op):
        p, fn, ctx = op.probs, self.fn, op.e.ctx
        ctx.call("ssdseg_loc_loss_iou", op.y_boxes, op.boxes.buf, fn.anchors_on(ctx), fn._stds, p.n, p.h * p.w, self.kind, fn.smooth_l1_weight,
                 op.w_loc / p.n, op.loc_loss, op.boxes.grad if op.e.training else None)


# the one table from a loss callable -- itself, or its `loss_kind` -- to (LossBinding kind, variant)
LOSSES = {
    LS.confidence_loss: ("conf", lambda *_: Mined()),           # these two fit any detection output: no check today, none added
    LS.localization_loss: ("loc", lambda *_: SmoothL1()),
    "focal": ("conf", Focal),
    "iou_loc": ("loc", IouLoc),
    "cross_entropy": ("mask", CrossEntropy),
    "dice": ("mask", Dice),
    "dice_square": ("mask", partial(Dice, squared=1)),
    "bootstrapped_cross_entropy": ("mask", lambda fn, *args: (BootstrappedVoid if _void_suffix(fn) else Bootstrapped)(fn, *args)),
}


def _row(fn):
    return LOSSES.get(fn if callable(fn) else None) or LOSSES.get(getattr(fn, "loss_kind", None)) or (None, None)


def _det_op(eng) -> DetLossOp:
    """the engine's detection loss op, created and emitted once: loaders and benchmarks hold its target buffers"""
    det = eng.loss_ops.get("det")
    if det is None:
        vals = [eng.vals[id(o)] for o in eng.model.outputs]
        labels_v = next(v for v in vals if "logits" in v.meta)
        boxes_v = next(v for v in vals if v.meta.get("head_concat"))
        det = eng.loss_ops["det"] = DetLossOp(eng, labels_v.meta["logits"], labels_v.store, boxes_v.store)
        eng._cur_reach = eng.DET_OUTPUTS
        eng._emit(det)
    return det


def bind_losses(eng, loss: dict, loss_weights: dict):
    """bind the compiled losses to the fused loss ops (reference NB03#cell14: cross_entropy(w) / confidence_loss /
    localization_loss, weights 1/1/1; Keras reduces each (B,) loss by its batch mean).  The binding state is
    rebuilt from this call's arguments alone: a loss or weight it does not name leaves nothing behind."""
    plan = []                                       # every error is raised here, before anything is bound
    for t in eng.model.outputs:
        name = t.layer.name
        fn = loss.get(name)
        if fn is None:
            continue
        v = eng.vals[id(t)]
        kind, variant = _row(fn)
        if "mask_head" in v.meta:
            if kind != "mask":
                raise NotImplementedError(f"loss for output {name}: the mask head trains with ssdseglib.losses.cross_entropy / dice / "
                                          "dice_square / bootstrapped_cross_entropy")
            impl = partial(variant, fn)             # allocates: made when it is bound
        elif kind in ("conf", "loc"):
            impl = variant(fn, name, v)
        else:
            raise NotImplementedError(f"loss for output {name}: only the ssdseglib.losses functions are supported")
        plan.append((name, kind, impl, fn, float(loss_weights.get(name, 1.0)), v))

    ctx, b = eng.ctx, eng.batch
    eng._loss_names = []
    eng.loaders.clear()                             # they hold the bindings' buffers
    det = _det_op(eng) if any(kind != "mask" for _, kind, *_ in plan) else eng.loss_ops.get("det")
    for op in eng.loss_ops.values():
        if op is det:
            det.conf_impl, det.loc_impl, det.w_conf, det.w_loc = Mined(), SmoothL1(), 1.0, 1.0
        else:
            op.unbind()
    for name, kind, impl, fn, w, v in plan:
        if kind == "mask":
            op: MaskHeadOp = v.meta["mask_head"]
            s = op.logits.store
            h, wd = s.h * op.fy, s.w * op.fx
            op.loss_impl = impl(ctx, b, h * wd)
            op.y_true = ctx.empty((b, h, wd, s.c))
            op.class_weights = LS.c4(fn.classes_weights)
            op.loss = ctx.empty(b)
            op.loss_scale = w / b
            eng._loss_names.append(LossBinding(name, op, "mask", op.y_true, op.loss, op.loss_scale * b))
        elif kind == "conf":
            det.conf_impl, det.w_conf = impl, w
            eng._loss_names.append(LossBinding(name, det, "conf", det.y_labels, det.conf_loss, w))
        else:
            det.loc_impl, det.w_loc = impl, w
            eng._loss_names.append(LossBinding(name, det, "loc", det.y_boxes, det.loc_loss, w))


# ====================================================================================================== metrics
def _mask_iou(ctx, fn, op, out):
    s = op.logits.store
    ctx.call("ssdseg_metric_mask_iou" + _void_suffix(fn), s.buf, s.n, s.h, s.w, s.c, op.fy, op.fx, 1, op.y_true, fn._cw, out)


def _label_accuracy(ctx, fn, op, out):
    p = op.probs
    ctx.call("ssdseg_metric_label_accuracy", op.y_labels, p.buf, p.n, p.h * p.w, p.c, fn._cw, out)


def _box_iou(ctx, fn, op, out):
    p = op.boxes
    ctx.call("ssdseg_metric_box_iou", op.y_boxes, p.buf, fn.anchors_on(ctx), fn._stds, p.n, p.h * p.w, out)


# `metric_kind` of a `metrics` callable -> (the LossBinding kind whose op and target buffer it shares, its launch)
METRICS = {"mask_iou": ("mask", _mask_iou), "label_accuracy": ("conf", _label_accuracy), "box_iou": ("loc", _box_iou)}


def bind_metrics(eng, metrics: dict):
    """bind compile(metrics={output: fn | [fn, ...]}) (NB03#cell14) to the device buffers of this engine's step: the
    ssdseglib.metrics callables are evaluated by `ssdseg_metric_*` right after the forward pass, from the same target
    buffers the losses use (needs bind_losses first); Keras naming `<output>_<function name>`"""
    bound = []
    targets = {r.name: (r.op, r.kind) for r in eng._loss_names}
    for t in eng.model.outputs:
        name = t.layer.name
        fns = metrics.get(name)
        if fns is None:
            continue
        for fn in (fns if isinstance(fns, (list, tuple)) else [fns]):
            kind = getattr(fn, "metric_kind", None)
            if kind is None:
                raise NotImplementedError(f"metric for output {name}: only the ssdseglib.metrics factories are supported")
            if name not in targets:
                raise NotImplementedError(f"metric for output {name} needs a compiled loss on the same output (it shares its target buffer)")
            op, lkind = targets[name]
            if METRICS[kind][0] != lkind:
                raise ValueError(f"metric {fn.__name__} does not fit output {name}")
            bound.append((f"{name}_{fn.__name__}", kind, fn, op, eng.ctx.empty(eng.batch)))
    eng._metrics = bound


def launch_metrics(eng):
    """launch the metric kernels on the outputs of the forward pass just run (asynchronous; read by `Engine.losses`)"""
    for key, kind, fn, op, out in eng._metrics:
        METRICS[kind][1](eng.ctx, fn, op, out)
