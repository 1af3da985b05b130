"""Void pixels in the mask losses and metrics, and the hard confusion matrix: float64 references, cases and derived bounds.  Plain NumPy.

A pixel is LABELLED iff any component of its y_true row is non-zero, otherwise VOID; L_i is the number of labelled pixels of image
i.  The entry points are ssdseg_mask_head_fwd_dice_void / _bwd_dice_void / _fwd_bootstrap_void / _bwd_bootstrap_void,
ssdseg_bootstrap_ce_loss_void, ssdseg_metric_mask_iou_void (csrc/mask_head.hip), ssdseg_dice_loss_void (csrc/losses.hip) and
ssdseg_eval_mask_scores (csrc/evaluate.hip).  tests/test_cpu_void_cases.py vets the references on the CPU against the plain ones
(oracle.np_ops through tests/_mask_cases.py, tests/_bootstrap_oracle.py) and by finite differences; tests/test_gpu_mask_void.py and
tests/test_gpu_eval_confusion.py run the kernels on the same cases.  Every builder seeds its own generator from its arguments.

The spec, restated here in float64:
  dice / dice_square   I_c = sum y_c p_c;  T_c = sum over LABELLED pixels of (y_c + p_c)  [y_c^2 + p_c^2];  loss, A_c, B_c from I, T
                       as mask_dice_final_kernel forms them;  dL/dp of a void pixel is a zero row;  L = 0: loss exactly 0
  bootstrapped         keep_i = min(L_i, max(1, ceil(keep_fraction L_i))) in double;  loss = sum of the labelled l >= the keep_i-th
                       largest labelled l (ties kept);  void is never kept;  L = 0: loss 0, kept 0, thresh +inf
  soft Jaccard         inter as before;  total = sum over labelled pixels of (y + p)
  confusion            labelled pixel of class k < C: M[k][argmax_c p_c] += 1 (lowest index on ties);  index >= C: void, no row

Bounds.  Inputs live on the lattice of tests/_mask_cases.py (logits are multiples of 1/4, factors powers of two), so the up-sampled
logits carry no error and the probabilities carry MC.prob_ref's bound.  The void paths add NO rounding to their plain twins: a void
pixel's probabilities are SELECTED to zero before they enter T_c (and s + 0 = s exactly), its dL/dp row is selected to zero, its
stored pixel loss is the constant -1.  Every float comparison therefore uses the plain case's derived bound, evaluated on what the
void path actually sums -- the probabilities and their bounds with the void rows zeroed -- and a void pixel's own outputs have
bound 0.  The one sum the plain suite bounds only through the cross-entropy's (the bootstrapped loss, "another summation of the same
terms") gets its own chain length here, see bootstrap_sum_bound.
"""
import math

import numpy as np

import _mask_cases as MC
import _tail_cases as TC
from oracle import np_ops as O

F32 = np.float32
U, gamma, seeded, w64 = MC.U, MC.gamma, MC.seeded, MC.w64
lattice, softmax_bound = MC.lattice, TC.softmax_bound
CW = MC.CW
KEPS = TC.KEPS32
VOID_LOSS = -1.0                         # what the device stores as a void pixel's loss

# (n, h, w, fy, fx): x4 with one partial tile, x4 with several tiles (TL = 16) and a partial one, x8 with partial tiles (TL = 8), and the
# gather kernel at x2 and x1
X4_SHAPES = [(1, 3, 5, 4, 4), (3, 17, 18, 4, 4)]
X8_SHAPES = [(2, 9, 10, 8, 8)]
GATHER_SHAPES = [(2, 3, 5, 2, 2), (2, 3, 5, 1, 1)]
SHAPES = X4_SHAPES + X8_SHAPES + GATHER_SHAPES
PATTERNS = ("none", "image", "single", "rect", "scattered")
FAMILY = "moderate"                      # |logit| <= 6: no probability near either end of the clip interval
KEEP_FRACTIONS = (0.25, 1.0, 1e-9)


def tag(shape):
    return "x".join(str(s) for s in shape)


def tile_edge(size, f):
    """the full-resolution index of the first tile border of an axis of `size` low-resolution pixels (the tile kernels' TL), or the
    middle of an axis that fits one tile"""
    tl = {4: MC.TL4, 8: MC.TL8}.get(f, size)
    return (tl if size > tl else max(1, size // 2)) * f


def labelled(y):
    """(n, npix) bool"""
    return (np.asarray(y) != 0).any(axis=-1)


def void_mask(shape, pattern):
    """(n, ho, wo) bool, True where the pixel is void.  none: no void pixel; image: one image entirely void (the second one where
    there are several, so that it stands beside labelled ones); single: one labelled pixel per image; rect: the rectangle from the
    image's top left corner (two edges on the image border) to the first tile border of each axis (two edges on a tile border);
    scattered: a seeded draw, about a third"""
    n, h, w, fy, fx = shape
    ho, wo = h * fy, w * fx
    void = np.zeros((n, ho, wo), bool)
    rng = seeded(71, n, h, w, fy, fx, PATTERNS.index(pattern))
    if pattern == "image":
        void[min(1, n - 1)] = True
    elif pattern == "single":
        void[:] = True
        for i in range(n):
            void[i, rng.integers(0, ho), rng.integers(0, wo)] = False
    elif pattern == "rect":
        void[:, :tile_edge(h, fy), :tile_edge(w, fx)] = True
    elif pattern == "scattered":
        void = rng.random((n, ho, wo)) < 1 / 3
    return void


def void_case(shape, pattern):
    """dict(logits, y, p, bp, shape, void): lattice logits of the moderate family, one-hot labels with the pattern's void rows"""
    n, h, w, fy, fx = shape
    void = void_mask(shape, pattern)
    y = TC.one_hot_rows(seeded(72, n, h, w, fy, fx), (n, h * fy * w * fx))
    y[void.reshape(n, -1)] = 0.0
    logits = MC.mask_logits(shape, FAMILY, 0)
    p, bp = MC.prob_ref(logits, fy, fx, FAMILY)
    assert not MC.undecidable(y, p, bp).any()
    return dict(logits=logits, y=y, p=p, bp=bp, shape=shape, void=void.reshape(n, -1), family=FAMILY, seed=0)


def masked(case):
    """(p, bp) with the void rows zeroed: what the void paths sum, and its error"""
    lab = labelled(case["y"])[..., None]
    return case["p"] * lab, case["bp"] * lab


def reach(case):
    """(n, h, w) bool: the low-resolution pixels whose interpolation window holds a labelled pixel; the others' gradient is +0"""
    n, h, w, fy, fx = case["shape"]
    lab = labelled(case["y"]).reshape(n, h * fy, w * fx, 1).astype(np.float64)
    return MC.down(lab, (MC.axis_weights(h, fy) != 0).astype(np.float64), (MC.axis_weights(w, fx) != 0).astype(np.float64))[..., 0] > 0


# ------------------------------------------------------------------------------------------------- dice / dice_square
def dice_void_sums(y, p, squared):
    y64 = y.astype(np.float64)
    lab = labelled(y)[..., None]
    return (y64 * p).sum(1), (((y64 * y64 + p * p) if squared else (y64 + p)) * lab).sum(1)


def dice_void_ref(y, p, weights, squared):
    """(loss (n,), coef (n, 8) = (A_c, B_c)) with T over the labelled pixels"""
    w = w64(weights)
    inter, total = dice_void_sums(y, p, squared)
    den, num = total + KEPS, 2 * inter + KEPS
    return (w * (1 - num / den)).sum(-1), np.concatenate([-2 * w / den, w * num / den ** 2], axis=-1)


def dice_void_dp(y, p, coef, squared):
    """dL/dp = A y + B [2 p] on labelled pixels, a zero row on void ones"""
    t = 2 * p if squared else np.ones_like(p)
    return (coef[:, None, :4] * y.astype(np.float64) + coef[:, None, 4:] * t) * labelled(y)[..., None]


def dice_void_bound(case, weights, squared):
    """MC.dice_bound on the masked probabilities: the sums hold the labelled terms and exact zeros"""
    pm, bpm = masked(case)
    return MC.dice_bound(case["y"], pm, bpm, weights, squared)


def dice_void_coef_error(case, weights, squared):
    pm, bpm = masked(case)
    return MC.SECOND_ORDER * MC.dice_coef_error(case["y"], pm, bpm, weights, squared)


def dice_void_backward(case, weights, squared, loss_scale):
    """(dlogits, bound): MC.dice_backward with the coefficients' errors taken from the masked sums and dL/dp -- value and error --
    zero on void rows (a select, no rounding); dz_bound gives such a row the bound 0"""
    y, p, bp = case["y"], case["p"], case["bp"]
    pm, bpm = masked(case)
    lab = labelled(y)[..., None]
    _, coef = dice_void_ref(y, p, weights, squared)
    dcoef = MC.dice_coef_error(y, pm, bpm, weights, squared)
    dp = dice_void_dp(y, p, coef, squared)
    t = 2 * p if squared else np.ones_like(p)
    ddp = lab * (dcoef[:, None, :4] * np.abs(y) + dcoef[:, None, 4:] * t + (np.abs(coef[:, None, 4:]) * 2 * bp if squared else 0.0)
                 + 2 * U * (np.abs(coef[:, None, :4] * y) + np.abs(coef[:, None, 4:] * t)))
    dz = MC.dz_of(p, dp)
    return MC.dlogits_ref(dz, case["shape"], loss_scale), MC.dlogits_bound(dz, MC.dz_bound(p, bp, dp, ddp), case["shape"], loss_scale)


def dice_loss_void_bound(y, p, weights, squared):
    """the standalone ssdseg_dice_loss_void from given float32 probabilities: TC.dice_bound on the masked probabilities"""
    return TC.dice_bound(y, np.asarray(p, np.float64) * labelled(y)[..., None], weights, int(squared))


# ------------------------------------------------------------------------------------------------- bootstrapped cross-entropy
def keep_void(keep_fraction, labelled_pixels):
    """min(L, max(1, ceil(keep_fraction L))) in double; 0 for L = 0"""
    l = int(labelled_pixels)
    return min(l, max(1, math.ceil(float(keep_fraction) * l)))


def bootstrap_void_ref(y, p, weights, keep_fraction, keep_mask=None):
    """-> dict(loss (n,), dp (n, npix, 4), mask (n, npix) bool, thresh (n,), keep (n,), kept (n,), l (n, npix)).  l: the labelled
    pixels' cross-entropy terms (MC.ce_pixel_ref), VOID_LOSS on void pixels.  keep_mask: take this selection (the device's) instead
    of the reference's own, for the loss and the gradient"""
    lab = labelled(y)
    l = np.where(lab, MC.ce_pixel_ref(y, p, weights), VOID_LOSS)
    n = y.shape[0]
    keep = np.array([keep_void(keep_fraction, lab[i].sum()) for i in range(n)], np.int32)
    thresh = np.array([np.sort(l[i][lab[i]])[::-1][keep[i] - 1] if keep[i] else np.inf for i in range(n)])
    mask = lab & (l >= thresh[:, None]) if keep_mask is None else np.asarray(keep_mask, bool)
    assert not (mask & ~lab).any()
    loss = np.where(mask, l, 0.0).sum(1)
    dp = MC.ce_dp(y, p, weights) * mask[..., None]
    return dict(loss=loss, dp=dp, mask=mask, thresh=thresh, keep=keep, kept=mask.sum(1).astype(np.int32), l=l)


def pixel_loss_bound(case, weights):
    """(n, npix): the cross-entropy's bound with one pixel per image (a chain of one), as the plain bootstrapped suite takes it; a void
    pixel's stored constant is exact"""
    y, p, bp = case["y"], case["p"], case["bp"]
    n, npix = y.shape[:2]
    b = MC.ce_bound(y.reshape(-1, 1, 4), p.reshape(-1, 1, 4), bp.reshape(-1, 1, 4), weights).reshape(n, npix)
    return b * labelled(y)


def bootstrap_blocks(npix):
    """mirror of bootstrap_blocks in csrc/mask_head.hip: blocks per image of the select and the sum pass, and a thread's trips"""
    nblk = min(32, -(-npix // 4096))
    return dict(nblk=nblk, trips=-(-npix // (nblk * 256)) + 3)       # (+ 3: a thread's last float4 may hold three more)


def bootstrap_sum_bound(l_ref, mask, term_bound):
    """the kept sum: every kept l carries its own bound; bootstrap_sum_kernel adds a thread's `trips` values, the block tree has 8
    levels, the fold is in double and its cast one rounding: gamma(trips + 8 + 1) of the sum of the kept (non-negative) l"""
    la = bootstrap_blocks(l_ref.shape[1])
    kept = np.where(mask, l_ref, 0.0)
    return MC.SECOND_ORDER * ((term_bound * mask).sum(1) + gamma(la["trips"] + 8 + 1) * kept.sum(1))


def bootstrap_void_backward(case, weights, keep_mask, loss_scale):
    """(dlogits, bound) with the selection `keep_mask`: the cross-entropy's backward (MC.ce_backward) of the labels with the
    dropped and the void rows zeroed -- a dropped pixel's dL/dp is selected to zero, no rounding"""
    kept = dict(case, y=case["y"] * np.asarray(keep_mask, bool)[..., None].astype(F32))
    return MC.ce_backward(kept, weights, loss_scale)


# ------------------------------------------------------------------------------------------------- soft Jaccard
def iou_void_ref(y, p, weights):
    y64, p64 = y.astype(np.float64), np.asarray(p, np.float64)
    inter = (y64 * p64).sum(1)
    total = ((y64 + p64) * labelled(y)[..., None]).sum(1)
    return (w64(weights) * inter / (total - inter + KEPS)).sum(-1)


def iou_void_bound(y, p, weights, perr=0.0):
    """TC.iou_bound on the masked probabilities"""
    return TC.iou_bound(y, np.asarray(p, np.float64) * labelled(y)[..., None], weights, perr)


# ------------------------------------------------------------------------------------------------- evaluation: Jaccard + confusion
def eval_case(n, hw, c, seed=0):
    """(prob (n, hw, c) float32, index (n, hw) uint8): probabilities k_j / sum k of small integers k (equal k are exact ties; a
    third of the pixels are forced to a tie of the leading classes), indices in 0 .. c + 1 (two void values) and 255, one void
    pixel for certain (from two pixels on), the last image all void where there are several"""
    rng = seeded(73, n, hw, c, seed)
    k = rng.integers(0, 5, (n, hw, c)).astype(np.float64)
    k[..., 0] += (k.sum(-1) == 0)
    prob = (k / k.sum(-1, keepdims=True)).astype(F32)
    tie = rng.random((n, hw)) < 1 / 3
    flat = np.full((c,), 1.0 / c, F32)
    prob[tie] = flat if c in (1, 2, 4, 8) else np.concatenate([[F32(0.5), F32(0.5)], np.zeros(c - 2, F32)])
    index = rng.integers(0, c + 2, (n, hw)).astype(np.uint8)
    index[rng.random((n, hw)) < 0.05] = 255
    if hw > 1:
        index[0, hw // 2] = c
    if n > 1:
        index[-1] = np.where(np.arange(hw) % 2 == 0, c, 255)
    return prob, index


def jaccard_ref(prob, index, c, ignore_void):
    """(n, c) float64: evaluators.jaccard_iou_semantic_segmentation's arithmetic per image, total over the labelled pixels only
    when ignore_void"""
    p = prob.astype(np.float64)
    y = (index[..., None] == np.arange(c)).astype(np.float64)
    lab = (index < c)[..., None] if ignore_void else 1.0
    inter, total = (y * p).sum(1), ((y + p) * lab).sum(1)
    return inter / (total - inter + 1e-7)


def confusion_ref(prob, index, c):
    """(M (n, c, c) int64, void (n,)) per image, a plain loop over np.argmax: rows true, columns predicted"""
    n, hw = index.shape
    m, void = np.zeros((n, c, c), np.int64), np.zeros(n, np.int64)
    pred = prob.argmax(-1)
    for i in range(n):
        for k, j in zip(index[i], pred[i]):
            if k < c:
                m[i, k, j] += 1
            else:
                void[i] += 1
    return m, void
