"""Training losses with the reference's API (reference losses.py): every function maps (y_true, y_pred) to one loss
value per batch item, shape (batch,).  Called directly they run the HIP kernels on cuda:0 and return NumPy arrays;
passed to `model.compile(loss={...})` they select the fused loss ops of the engine (`_loss_bind.bind_losses`),
where the gradient comes out of the same launch.
"""
import ctypes as C
import math
from typing import Callable, List

import numpy as np


# ---------------------------------------------------------------- what the standalone callables here and in `metrics` share
def _ctx():
    from . import _engine
    return _engine.default_context()


def c4(values):
    """four floats as the host array the C entries take (class weights, alpha, standard deviations)"""
    return (C.c_float * 4)(*[float(v) for v in values])


def shape_of(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def dev(a):
    """`a` on the default context: a device buffer as it is, anything else uploaded as float32"""
    from . import _hip as H
    return a if isinstance(a, H.DeviceBuffer) else _ctx().array(np.ascontiguousarray(a, dtype=np.float32))


OUT = object()      # among `per_sample`'s arguments: the place of the (batch,) result


def per_sample(entry: str, batch: int, *args) -> np.ndarray:
    """call the compiled `entry` on the default context and download the one value per batch item it writes"""
    ctx = _ctx()
    out = ctx.empty(batch)
    ctx.call(entry, *[out if a is OUT else a for a in args])
    return out.download()


def boxes_on_context(anchors: np.ndarray) -> Callable:
    """-> anchors_on(ctx): the default boxes [a][4] = cx, cy, w, h on `ctx`'s device, uploaded once per context (data-parallel
    ranks each have one)"""
    state = {}

    def anchors_on(ctx):
        if id(ctx) not in state:
            state[id(ctx)] = (ctx, ctx.array(anchors))
        return state[id(ctx)][1]

    return anchors_on


# -------------------------------------------------------------------------------------------------------------- the losses
def localization_loss(y_true, y_pred):
    """smooth-L1 over non-background anchors / max(#non-background, 1) (reference losses.py:21-49)."""
    b, a, _ = shape_of(y_true)
    dummy_labels = np.zeros((b, a, 4), np.float32)
    dummy_labels[..., 0] = 1.0
    return per_sample("ssdseg_det_loss", b, dev(dummy_labels), dev(np.full((b, a, 4), 0.25, np.float32)), dev(y_true), dev(y_pred),
                      b, a, 4, 1.0, None, OUT, None, None, None)


def confidence_loss(y_true, y_pred):
    """softmax cross-entropy with batch-global 3:1 hard-negative mining (reference losses.py:70-172);
    y_pred are probabilities."""
    b, a, c = shape_of(y_true)
    zeros = _ctx().zeros((b, a, 4))
    return per_sample("ssdseg_det_loss", b, dev(y_true), dev(y_pred), zeros, zeros, b, a, c, 1.0, OUT, None, None, None, None)


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
        b, a, c = shape_of(y_true)
        zeros = _ctx().zeros((b, a, 4))
        return per_sample("ssdseg_det_loss_focal", b, dev(y_true), dev(y_pred), zeros, zeros, b, a, c, c4(weights), gamma, 1.0, 1.0,
                          OUT, None, None, None)

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
    cstds, anchors_on = c4(stds), boxes_on_context(anchors)

    def loss_fn(y_true, y_pred):
        b, a, _ = shape_of(y_true)
        if a != anchors.shape[0]:
            raise ValueError(f"{a} boxes per image, {anchors.shape[0]} default boxes")
        return per_sample("ssdseg_loc_loss_iou", b, dev(y_true), dev(y_pred), anchors_on(_ctx()), cstds, b, a, IOU_KINDS[kind], weight, 1.0,
                          OUT, None)

    loss_fn.__name__ = "iou_localization_loss"
    loss_fn.loss_kind = "iou_loc"
    loss_fn.kind, loss_fn.smooth_l1_weight = kind, weight
    loss_fn.anchors_on, loss_fn.n_anchors, loss_fn._stds = anchors_on, anchors.shape[0], cstds
    return loss_fn


def void_flag(ignore_void) -> bool:
    """the `ignore_void` option of the mask losses and of the mask metric: a bool, nothing that merely converts to one"""
    if not isinstance(ignore_void, (bool, np.bool_)):
        raise ValueError(f"ignore_void must be a bool, got {ignore_void!r}")
    return bool(ignore_void)


def _mask_loss(mode: int, name: str, kind: str, classes_weights: List[float], ignore_void: bool = False) -> Callable:
    weights = tuple(float(w) for w in classes_weights)
    entry = "ssdseg_dice_loss_void" if void_flag(ignore_void) else "ssdseg_dice_loss"

    def loss_fn(y_true, y_pred):
        n, *hw, c = shape_of(y_true)
        return per_sample(entry, n, dev(y_true), dev(y_pred), n, int(np.prod(hw)), c, c4(weights), mode, OUT)

    loss_fn.__name__ = name
    loss_fn.classes_weights = weights
    loss_fn.loss_kind = kind
    loss_fn.ignore_void = bool(ignore_void)
    return loss_fn


def bootstrap_keep(keep_fraction: float, pixels: int) -> int:
    """pixels kept per image by `bootstrapped_cross_entropy`: ceil(keep_fraction * pixels) in double, at least 1, at most all"""
    return min(int(pixels), max(1, math.ceil(float(keep_fraction) * int(pixels))))


def bootstrapped_cross_entropy(classes_weights: List[float], keep_fraction: float = 0.25, ignore_void: bool = False) -> Callable:
    """weighted pixel cross-entropy over the hardest pixels of each image only (hard-pixel mining, DeepLab's bootstrapped
    cross-entropy; not in the reference): with l_i = -sum_c w_c y_ic log(clip p_ic) the `cross_entropy` term of pixel i and
    keep = min(H W, max(1, ceil(keep_fraction H W))), an image's loss is the sum of the l_i >= its keep-th largest l.  Every pixel
    tied with the keep-th value is kept (no tie-break by index), so more than `keep` pixels may count.  The selection is per
    image: no image depends on the rest of its batch.  keep_fraction = 1 is `cross_entropy`.

    ignore_void=True: void pixels (all-zero y_true rows: a class index >= 4, the fill_class=255 padding of a crop or a mosaic) are
    never kept, and keep is formed per image ON THE DEVICE from L, the image's labelled pixels, in place of H W -- after a
    zoom-out that leaves 1/16 of the image labelled, keep_fraction=0.25 still mines a quarter of what is labelled.  An image
    without a labelled pixel has loss 0 and a zero gradient."""
    ignore_void = void_flag(ignore_void)
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
        n, *hw, c = shape_of(y_true)
        hw = int(np.prod(hw))
        if ignore_void:
            return per_sample("ssdseg_bootstrap_ce_loss_void", n, dev(y_true), dev(y_pred), n, hw, c, c4(weights), keep_fraction, OUT)
        return per_sample("ssdseg_bootstrap_ce_loss", n, dev(y_true), dev(y_pred), n, hw, c, c4(weights), bootstrap_keep(keep_fraction, hw), OUT)

    loss_fn.__name__ = "bootstrapped_cross_entropy_loss"
    loss_fn.classes_weights = weights
    loss_fn.keep_fraction = keep_fraction
    loss_fn.ignore_void = ignore_void
    loss_fn.loss_kind = "bootstrapped_cross_entropy"
    return loss_fn


def dice(classes_weights: List[float], ignore_void: bool = False) -> Callable:
    """weighted dice loss on probabilities (reference losses.py:204-216).  ignore_void=True: a void pixel (all-zero y_true row) is
    left out of T_c = sum (y_c + p_c) and gets a zero gradient; as the reference has it, its probabilities count as false
    positives of every class."""
    return _mask_loss(0, "dice_loss", "dice", classes_weights, ignore_void)


def dice_square(classes_weights: List[float], ignore_void: bool = False) -> Callable:
    """weighted squared-denominator dice loss (reference losses.py:250-262).  ignore_void: as `dice`."""
    return _mask_loss(1, "dice_square_loss", "dice_square", classes_weights, ignore_void)


def cross_entropy(classes_weights: List[float]) -> Callable:
    """weighted pixel cross-entropy on probabilities, summed over pixels and classes (reference losses.py:294-305);
    the loss NB03#cell10 trains the mask head with.  It ignores void pixels as it stands: an all-zero y_true row has a zero term
    and a zero gradient, so it takes no `ignore_void` option."""
    return _mask_loss(2, "cross_entropy_loss", "cross_entropy", classes_weights)
