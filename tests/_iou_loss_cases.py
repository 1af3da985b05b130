"""Inputs of the IoU-family box loss tests (`ssdseg_loc_loss_iou`), one builder for the CPU and the GPU file.

Default boxes: the project's `DefaultBoundingBoxes` of the 480 x 640 model (9600 anchors) for a = 9600, an evenly strided slice of
them otherwise, so every feature map's box sizes (27 .. 671 px) occur at every a.  Targets of the box-carrying anchors have
positive decoded sizes (t.z, t.w = log(1 + r) / s with r in [0.3, 3]) and centres within 0.3 default-box sizes; the other
anchors' targets are exactly zero.  Predictions: "near" = t + N(0, 0.8) on every component, "init" = N(0, 0.05), an untrained head
(decoded sizes around zero, of either sign).

The seeds are fixed and were picked on the CPU so that every box-carrying anchor of every case keeps clear of every kink of the
loss (`kink_margins`, asserted by test_cpu_iou_loss_oracle.py): float32 and float64 then take the same branch at every min, max,
clamp and smooth-L1 knee, and no anchor has to be left out of a comparison.

F32_LOSS_REL / F32_DBOX_ABS: the worst error of the spec evaluated in float32 NumPy against the spec in float64 on these
inputs (float32 inputs to both), over every case, kind and smooth_l1_weight in {0, 1}: relative error of the loss, and absolute
error of d_boxes over the case's max |d_boxes|.  Measured and pinned by test_cpu_iou_loss_oracle.py; the GPU test allows 4 x
these (the device's expf, its division and its different reduction order), not anything derived from the kernel.
"""
import functools

import numpy as np

STDS = (0.1, 0.1, 0.2, 0.2)
KIND_NAMES = ("iou", "giou", "diou")
LAMBDAS = (0.0, 1.0)
SHAPES = [(4, 600, 0.03),      # ordinary case
          (3, 500, 0.0),       # no object anywhere: loss and gradient exactly zero
          (2, 300, 0.6),       # many box anchors
          (1, 37, 0.1),        # fewer anchors than blocks per image: empty blocks, ragged chunk
          (2, 9600, 0.01)]     # the real anchor count
SETS = ("near", "init")
SEEDS = {(b, a, f, which): 1993 for (b, a, f) in SHAPES for which in SETS}
SEEDS[(2, 9600, 0.01, "init")] = 1994      # seed 1993 puts one anchor 6e-4 px from a kink

F32_LOSS_REL = 4.4e-7
F32_DBOX_ABS = 4.1e-5

MARGIN_PX, MARGIN_KNEE = 1e-3, 1e-4


@functools.lru_cache(maxsize=None)
def all_default_boxes():
    """(9600, 4) float32 = cx, cy, w, h of the 480 x 640 model's default boxes (NB03#cell6)"""
    from ssdseglib.boxes import DefaultBoundingBoxes
    boxes = DefaultBoundingBoxes(feature_maps_shapes=((30, 40), (15, 20), (8, 10), (4, 5)),
                                 centers_padding_from_borders_percentage=(0.025, 0.05, 0.075, 0.1), boxes_scales=(0.15, 0.95),
                                 additional_square_box=True)
    boxes.rescale_boxes_coordinates(image_shape=(480, 640))
    cent = np.stack([np.asarray(getattr(boxes, f"get_boxes_coordinates_{k}")("ssd"), np.float32).reshape(-1)
                     for k in ("center_x", "center_y", "width", "height")], axis=1)
    assert cent.shape == (9600, 4)
    cent.setflags(write=False)
    return cent


def default_boxes(a):
    full = all_default_boxes()
    out = np.ascontiguousarray(full[(np.arange(a) * full.shape[0]) // a])
    out.setflags(write=False)
    return out


def make_case(seed, b, a, pos_frac, which):
    """-> t, p (b, a, 4) float32, anchors (a, 4) float32"""
    rng = np.random.default_rng(seed)
    box = rng.uniform(size=(b, a)) < pos_frac
    t = np.empty((b, a, 4))
    t[..., :2] = rng.uniform(-3, 3, (b, a, 2))
    t[..., 2:] = np.log1p(rng.uniform(0.3, 3.0, (b, a, 2))) / np.asarray(STDS[2:])
    t = (t * box[..., None]).astype(np.float32)
    if which == "near":
        p = (t + rng.normal(0, 0.8, (b, a, 4))).astype(np.float32)
    else:
        assert which == "init", which
        p = rng.normal(0, 0.05, (b, a, 4)).astype(np.float32)
    return t, p, default_boxes(a)


@functools.lru_cache(maxsize=None)
def case(b, a, pos_frac, which):
    """the shared, read-only inputs of one shape and prediction set"""
    arrays = make_case(SEEDS[(b, a, pos_frac, which)], b, a, pos_frac, which)
    for v in arrays:
        v.setflags(write=False)
    return arrays


def kink_margins(t, p, anchors, stds=STDS):
    """smallest distance of a box-carrying anchor from a kink, in float64 on the given inputs: (pixels between the operands of any
    min / max / clamp, raw decoded sizes and raw intersection extents against 0 included; | |t - p| - 1 | of the smooth-L1 knee).
    (inf, inf) without a box-carrying anchor."""
    import _iou_loss_oracle as S
    t64, p64, an = np.asarray(t, np.float64), np.asarray(p, np.float64), np.asarray(anchors, np.float64)
    box = np.abs(t64).sum(-1) > 0
    if not box.any():
        return np.inf, np.inf
    g, q = S.decode(t64, an, stds), S.decode(p64, an, stds)
    px = [np.abs(q[k] - g[k]) for k in ("x0", "y0", "x1", "y1")]                                    # every min / max of two corners
    px += [np.abs(d[k]) for d in (g, q) for k in ("rw", "rh")]                                     # the size clamps
    for lo, hi, size in (("x0", "x1", "w"), ("y0", "y1", "h")):                                    # the intersection clamps
        raw = np.minimum(q[hi], g[hi]) - np.maximum(q[lo], g[lo])
        # a predicted size clamped to 0 inside the target's span: lo == hi == the centre, the raw extent is c - c = 0 in every
        # precision (not a value near a kink but the clamp's own branch, taken alike by float32 and float64)
        px.append(np.where((q[size] == 0) & (raw == 0), np.inf, np.abs(raw)))
    knee = np.abs(np.abs(t64 - p64) - 1.0)
    return float(min(v[box].min() for v in px)), float(knee[box].min())


def tie_case():
    """(2, 300, 0.6) "near" with every second box-carrying anchor's prediction bit-equal to its target: every min / max of those
    rows is a tie"""
    t, p, anchors = case(2, 300, 0.6, "near")
    p = p.copy()
    rows = np.argwhere(np.abs(t).sum(-1) > 0)[::2]
    p[rows[:, 0], rows[:, 1]] = t[rows[:, 0], rows[:, 1]]
    p.setflags(write=False)
    return t, p, anchors, rows


def clamp_case():
    """(4, 600, 0.03) "init": an untrained head, about half of the raw predicted sizes negative -- the clamp case"""
    return case(4, 600, 0.03, "init")
