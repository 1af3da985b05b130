"""fp64 NumPy specification of the bootstrapped cross-entropy (hard-pixel mining) of the mask head, built on oracle.np_ops.

For pixel i of image b, with one-hot y, class weights w >= 0 and probabilities p:
    l_i    = -sum_c w_c y_ic clip_log(p_ic)             (the term oracle.np_ops.cross_entropy_loss sums)
    tau_b  = the keep-th largest l of image b,  1 <= keep <= H W
    keep_i = [l_i >= tau_b]                              (EVERY pixel tied with the keep-th value: the count may exceed keep)
    loss_b = sum_i keep_i l_i
    dL_b/dp_i = the cross-entropy's for kept pixels, an exact zero row for dropped ones

The functions follow the dtype of `p` like the rest of oracle.np_ops, so the float32 restatement of the device's arithmetic
is the same text run on float32 arrays."""
import math

import numpy as np

from oracle import np_ops as O


def keep_count(keep_fraction, pixels):
    """min(H W, max(1, ceil(keep_fraction H W))), in double"""
    return min(int(pixels), max(1, math.ceil(float(keep_fraction) * int(pixels))))


def pixel_losses(y, p, w):
    """l (B, H, W) in p's dtype"""
    logp, _ = O._clipped_log(p)
    return -(y.astype(p.dtype) * logp * np.asarray(w, p.dtype)).sum(axis=-1)


def thresholds(l, keep):
    """(B,) the keep-th largest l of every image"""
    flat = l.reshape(l.shape[0], -1)
    assert 1 <= keep <= flat.shape[1]
    return np.partition(flat, flat.shape[1] - keep, axis=1)[:, flat.shape[1] - keep]


def with_keep_mask(y, p, w, keep_mask):
    """(loss (B,), dL/dp) of the cross-entropy restricted to the pixels of `keep_mask` (B, H, W), whoever selected them"""
    # a dropped pixel adds nothing to the loss and has a zero gradient row: the cross-entropy of the target with its row zeroed
    # (with every pixel kept this IS oracle.np_ops.cross_entropy_loss, summation order included)
    keep_mask = np.asarray(keep_mask, bool).reshape(p.shape[:-1])
    return O.cross_entropy_loss(y.astype(p.dtype) * keep_mask[..., None], p, w)


def bootstrapped_cross_entropy(y, p, w, keep):
    """-> (loss (B,), dL/dp (B, H, W, C), keep_mask (B, H, W) bool, thresh (B,))"""
    l = pixel_losses(y, p, w)
    thresh = thresholds(l, keep)
    keep_mask = l >= thresh.reshape((-1,) + (1,) * (l.ndim - 1))
    loss, dp = with_keep_mask(y, p, w, keep_mask)
    return loss, dp, keep_mask, thresh
