"""Training losses with the reference's API (reference losses.py): every function maps (y_true, y_pred) to one loss
value per batch item, shape (batch,).  Called directly they run the HIP kernels on cuda:0 and return NumPy arrays;
passed to `model.compile(loss={...})` they select the fused loss ops of the engine (`_engine.configure_losses`),
where the gradient comes out of the same launch.
"""
import ctypes as C
import math
from typing import Callable, List

import numpy as np


def _ctx():
    from . import _engine
    return _engine.default_context()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def localization_loss(y_true, y_pred):
    """smooth-L1 over non-background anchors / max(#non-background, 1) (reference losses.py:21-49)."""
    y_true, y_pred = _f32(y_true), _f32(y_pred)
    b, a, _ = y_true.shape
    ctx = _ctx()
    dummy_labels = np.zeros((b, a, 4), np.float32)
    dummy_labels[..., 0] = 1.0
    loc = ctx.empty(b)
    ctx.call("ssdseg_det_loss", ctx.array(dummy_labels), ctx.array(np.full((b, a, 4), 0.25, np.float32)), ctx.array(y_true), ctx.array(y_pred),
             b, a, 4, 1.0, None, loc, None, None, None)
    return loc.download()


def confidence_loss(y_true, y_pred):
    """softmax cross-entropy with batch-global 3:1 hard-negative mining (reference losses.py:70-172);
    y_pred are probabilities."""
    y_true, y_pred = _f32(y_true), _f32(y_pred)
    b, a, c = y_true.shape
    ctx = _ctx()
    zeros = ctx.zeros((b, a, 4))
    conf = ctx.empty(b)
    ctx.call("ssdseg_det_loss", ctx.array(y_true), ctx.array(y_pred), zeros, zeros, b, a, c, 1.0, conf, None, None, None, None)
    return conf.download()


def focal_confidence_loss(alpha=(1.0, 1.0, 1.0, 1.0), gamma: float = 2.0) -> Callable:
    """focal loss on the softmax probabilities of the SSD head (not in the reference): per anchor
    -sum_c alpha_c y_c (1 - p_c)^gamma log p_c with p clipped like `confidence_loss`, summed over EVERY anchor of an image
    (no hard-negative mining, so no image depends on the rest of its batch) / max(#non-background anchors, 1).
    alpha: one weight per class (background first), gamma >= 0; gamma = 0, alpha = 1 is the un-mined cross-entropy."""
    try:
        weights = tuple(float(w) for w in alpha)
    except TypeError:
        raise ValueError("alpha must hold one weight per class (4)") from None
    gamma = float(gamma)
    if len(weights) != 4:
        raise ValueError(f"alpha must hold one weight per class (4), got {len(weights)}")
    if not all(np.isfinite(w) and w >= 0.0 for w in weights):
        raise ValueError(f"alpha must be finite and >= 0, got {weights}")
    if not (np.isfinite(gamma) and gamma >= 0.0):
        raise ValueError(f"gamma must be finite and >= 0, got {gamma}")

    def loss_fn(y_true, y_pred):
        y_true, y_pred = _f32(y_true), _f32(y_pred)
        b, a, c = y_true.shape
        ctx = _ctx()
        zeros = ctx.zeros((b, a, 4))
        conf = ctx.empty(b)
        ctx.call("ssdseg_det_loss_focal", ctx.array(y_true), ctx.array(y_pred), zeros, zeros, b, a, c, (C.c_float * 4)(*weights), gamma, 1.0, 1.0,
                 conf, None, None, None)
        return conf.download()

    loss_fn.__name__ = "focal_confidence_loss"
    loss_fn.alpha = weights
    loss_fn.gamma = gamma
    loss_fn.loss_kind = "focal"
    return loss_fn


IOU_KINDS = {"iou": 0, "giou": 1, "diou": 2}


def iou_localization_loss(center_x_boxes_default, center_y_boxes_default, width_boxes_default, height_boxes_default,
                          standard_deviations_centroids_offsets, kind: str = "giou", smooth_l1_weight: float = 1.0) -> Callable:
    """IoU-family box regression loss of the SSD head (not in the reference), for `compile(loss={'output-boxes': ...})` in place
    of `localization_loss`: per image, over the anchors that carry a box (`localization_loss`'s own test),
    sum(smooth_l1_weight * smooth-L1 + term) / max(#box anchors, 1), where smooth-L1 is `localization_loss`'s and the term compares
    the DECODED target and predicted boxes: "iou" 1 - IoU, "giou" 1 - IoU + (E - U) / E with E the enclosing box's area, "diou"
    1 - IoU + squared centre distance / squared enclosing diagonal.  Both offsets decode alike against the default boxes (argument
    order of `metrics.jaccard_iou_bounding_boxes`): cx = o.x s.x aw + ax, w = max((exp(o.z s.z) - 1) aw, 0), corners cx -+ w/2.
    These are continuous boxes, without the `+1` / `(w - 1) / 2` pixel conventions of the metric and of the decode layer.

    Why smooth-L1 stays in (the DETR-style sum, weight 1 by default, 0 allowed): the decode gives an untrained head (offsets
    near 0, exactly 0 behind a dead ReLU6) boxes of near-zero size, and there a pure overlap loss has an exactly zero gradient on
    both size offsets for most box-carrying anchors (IoU 85 %, GIoU / DIoU 65 % in a float64 prototype on synthetic anchors; still
    5-18 % near the target).  With the smooth-L1 term no anchor is left without one."""
    if not isinstance(kind, str) or kind not in IOU_KINDS:
        raise ValueError(f"kind must be one of {sorted(IOU_KINDS)}, got {kind!r}")
    try:
        weight = float(smooth_l1_weight)
        stds = tuple(float(s) for s in standard_deviations_centroids_offsets)
        defaults = [np.asarray(v, np.float32).reshape(-1) for v in
                    (center_x_boxes_default, center_y_boxes_default, width_boxes_default, height_boxes_default)]
    except (TypeError, ValueError):
        raise ValueError("smooth_l1_weight must be a number, the stds four numbers, the default boxes four vectors of numbers") from None
    if not (np.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"smooth_l1_weight must be finite and >= 0, got {weight}")
    if len(stds) != 4 or not all(np.isfinite(s) and s > 0.0 for s in stds):
        raise ValueError(f"standard_deviations_centroids_offsets must hold four finite numbers > 0, got {stds}")
    if len({v.size for v in defaults}) != 1 or defaults[0].size == 0:
        raise ValueError(f"the default-box vectors must have one common length > 0, got {[v.size for v in defaults]}")
    anchors = np.ascontiguousarray(np.stack(defaults, axis=1))
    cstds = (C.c_float * 4)(*stds)
    state = {}

    def anchors_on(ctx):
        """the default boxes [a][4] = cx, cy, w, h on `ctx`'s device, uploaded once per context (data-parallel ranks each have one)"""
        if id(ctx) not in state:
            state[id(ctx)] = (ctx, ctx.array(anchors))
        return state[id(ctx)][1]

    def loss_fn(y_true, y_pred):
        y_true, y_pred = _f32(y_true), _f32(y_pred)
        b, a, _ = y_true.shape
        if a != anchors.shape[0]:
            raise ValueError(f"{a} boxes per image, {anchors.shape[0]} default boxes")
        ctx = _ctx()
        loc = ctx.empty(b)
        ctx.call("ssdseg_loc_loss_iou", ctx.array(y_true), ctx.array(y_pred), anchors_on(ctx), cstds, b, a, IOU_KINDS[kind], weight, 1.0, loc, None)
        return loc.download()

    loss_fn.__name__ = "iou_localization_loss"
    loss_fn.loss_kind = "iou_loc"
    loss_fn.kind, loss_fn.smooth_l1_weight = kind, weight
    loss_fn.anchors_on, loss_fn.n_anchors, loss_fn._stds = anchors_on, anchors.shape[0], cstds
    return loss_fn


def _mask_loss(mode: int, name: str, kind: str, classes_weights: List[float]) -> Callable:
    weights = tuple(float(w) for w in classes_weights)

    def loss_fn(y_true, y_pred):
        y_true, y_pred = _f32(y_true), _f32(y_pred)
        n, c = y_true.shape[0], y_true.shape[-1]
        hw = int(np.prod(y_true.shape[1:-1]))
        ctx = _ctx()
        out = ctx.empty(n)
        ctx.call("ssdseg_dice_loss", ctx.array(y_true), ctx.array(y_pred), n, hw, c, (C.c_float * 4)(*weights), mode, out)
        return out.download()

    loss_fn.__name__ = name
    loss_fn.classes_weights = weights
    loss_fn.loss_kind = kind
    return loss_fn


def bootstrap_keep(keep_fraction: float, pixels: int) -> int:
    """pixels kept per image by `bootstrapped_cross_entropy`: ceil(keep_fraction * pixels) in double, at least 1, at most all"""
    return min(int(pixels), max(1, math.ceil(float(keep_fraction) * int(pixels))))


def bootstrapped_cross_entropy(classes_weights: List[float], keep_fraction: float = 0.25) -> Callable:
    """weighted pixel cross-entropy over the hardest pixels of each image only (hard-pixel mining, DeepLab's bootstrapped
    cross-entropy; not in the reference): with l_i = -sum_c w_c y_ic log(clip p_ic) the `cross_entropy` term of pixel i and
    keep = min(H W, max(1, ceil(keep_fraction H W))), an image's loss is the sum of the l_i >= its keep-th largest l.  Every pixel
    tied with the keep-th value is kept (no tie-break by index), so more than `keep` pixels may count.  The selection is per
    image: no image depends on the rest of its batch.  keep_fraction = 1 is `cross_entropy`."""
    try:
        weights = tuple(float(w) for w in classes_weights)
    except TypeError:
        raise ValueError("classes_weights must hold one weight per class (4)") from None
    if len(weights) != 4:
        raise ValueError(f"classes_weights must hold one weight per class (4), got {len(weights)}")
    if not all(np.isfinite(w) and w >= 0.0 for w in weights):
        raise ValueError(f"classes_weights must be finite and >= 0, got {weights}")
    try:
        keep_fraction = float(keep_fraction)
    except TypeError:
        raise ValueError("keep_fraction must be a number in (0, 1]") from None
    if not (np.isfinite(keep_fraction) and 0.0 < keep_fraction <= 1.0):
        raise ValueError(f"keep_fraction must be finite and in (0, 1], got {keep_fraction}")

    def loss_fn(y_true, y_pred):
        y_true, y_pred = _f32(y_true), _f32(y_pred)
        n, c = y_true.shape[0], y_true.shape[-1]
        hw = int(np.prod(y_true.shape[1:-1]))
        ctx = _ctx()
        out = ctx.empty(n)
        ctx.call("ssdseg_bootstrap_ce_loss", ctx.array(y_true), ctx.array(y_pred), n, hw, c, (C.c_float * 4)(*weights), bootstrap_keep(keep_fraction, hw),
                 out)
        return out.download()

    loss_fn.__name__ = "bootstrapped_cross_entropy_loss"
    loss_fn.classes_weights = weights
    loss_fn.keep_fraction = keep_fraction
    loss_fn.loss_kind = "bootstrapped_cross_entropy"
    return loss_fn


def dice(classes_weights: List[float]) -> Callable:
    """weighted dice loss on probabilities (reference losses.py:204-216)."""
    return _mask_loss(0, "dice_loss", "dice", classes_weights)


def dice_square(classes_weights: List[float]) -> Callable:
    """weighted squared-denominator dice loss (reference losses.py:250-262)."""
    return _mask_loss(1, "dice_square_loss", "dice_square", classes_weights)


def cross_entropy(classes_weights: List[float]) -> Callable:
    """weighted pixel cross-entropy on probabilities, summed over pixels and classes (reference losses.py:294-305);
    the loss NB03#cell10 trains the mask head with."""
    return _mask_loss(2, "cross_entropy_loss", "cross_entropy", classes_weights)
