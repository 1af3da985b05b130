"""fp64 NumPy restatement of the focal confidence loss (`ssdseg_det_loss_focal`, `losses.focal_confidence_loss`).

With eps = 1e-7 and ph = clip(p, eps, 1 - eps):
    per anchor   FL = -sum_c alpha_c y_c (1 - ph_c)^gamma log ph_c
    per image    loss[i] = sum over ALL anchors of FL / max(#non-background anchors of image i, 1)
    dFL/dp_c     = -alpha_c y_c inside(p_c) [ (1 - ph_c)^gamma / ph_c - gamma (1 - ph_c)^(gamma - 1) log ph_c ]
The clip constants and `inside` are the project's (`oracle.np_ops._clipped_log`): formed in the dtype of `p`, so a float32 `p`
is clipped at the device's float32 constants (eps32 > 1e-7, 1 - 2^-23 < 1 - 1e-7) and a float64 `p` at the float64 ones.  All
arithmetic after the clip is float64.  test_cpu_focal_oracle.py pins this file (finite differences, torch autograd, the
cross-entropy limit); test_gpu_focal_loss.py pins the kernel to it.
"""
import numpy as np

from oracle import np_ops as O


def clip_and_inside(p):
    """(clip(p) as float64, inside(p) as float64) under the clip constants of p's dtype"""
    dt = p.dtype
    _, inside = O._clipped_log(p)
    lo, hi = np.asarray(O.EPS, dt), np.asarray(1.0, dt) - np.asarray(O.EPS, dt)      # as _clipped_log forms them
    return np.clip(p, lo, hi).astype(np.float64), inside.astype(np.float64)


def focal_confidence_loss(y, p, alpha, gamma):
    """-> loss (B,) float64, dL_b/dp (B, A, 4) float64 (the per-image normaliser included)"""
    p = np.asarray(p)
    y = np.asarray(y, np.float64)
    alpha = np.asarray(alpha, np.float64)
    gamma = float(gamma)
    assert alpha.shape == (4,) and (alpha >= 0).all() and np.isfinite(alpha).all() and gamma >= 0
    ph, inside = clip_and_inside(p)
    q = 1.0 - ph
    logp = np.log(ph)
    fl = -(alpha * y * q ** gamma * logp).sum(axis=-1)
    npos = np.maximum(np.abs(y[..., 0] - 1.0).sum(axis=-1), 1.0)
    loss = fl.sum(axis=-1) / npos
    slope = gamma * q ** (gamma - 1.0) * logp if gamma > 0 else np.zeros_like(q)
    dp = -alpha * y * inside * (q ** gamma / ph - slope) / npos[:, None, None]
    return loss, dp
