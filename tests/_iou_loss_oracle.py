"""NumPy restatement of the IoU-family box regression loss (`ssdseg_loc_loss_iou`, `losses.iou_localization_loss`), with its
analytic gradient through the decode.  float64 by default; `dtype=np.float32` runs the same expressions in float32 (the measure
of what single precision costs, test_cpu_iou_loss_oracle.py).

For image n, anchor i with default box (ax, ay, aw, ah), target offsets t, predicted offsets p, stds s:
    box      = 1 if |t.x| + |t.y| + |t.z| + |t.w| > 0 else 0                (localization_loss's own test)
    decode   cx = o.x s.x aw + ax,  cy = o.y s.y ah + ay,  w = max((exp(o.z s.z) - 1) aw, 0),  h = max((exp(o.w s.w) - 1) ah, 0),
             corners cx -+ w/2, cy -+ h/2, for o = t (box g) and o = p (box p) alike
    iw       = max(min(px1, gx1) - max(px0, gx0), 0), ih likewise;  I = iw ih;  U = pw ph + gw gh - I;  IoU = I / (U + 1e-7)
    ew       = max(px1, gx1) - min(px0, gx0), eh likewise
    term     kind 0 (IoU):  1 - IoU
             kind 1 (GIoU): 1 - IoU + (E - U) / (E + 1e-7),  E = ew eh
             kind 2 (DIoU): 1 - IoU + ((pcx - gcx)^2 + (pcy - gcy)^2) / (ew^2 + eh^2 + 1e-7)
    loss[n]  = sum_i box_i (lambda sl1_i + term_i) / max(sum_i box_i, 1),   sl1 = localization_loss's smooth-L1 of t - p
These are CONTINUOUS boxes: corners c -+ w/2 and areas w h, without the `+1` / `(w - 1) / 2` pixel conventions of
`metrics.jaccard_iou_bounding_boxes` and of the decode layer.  pw, ph, gw, gh are the decoded (clamped) sizes themselves.

Gradient with respect to p: at a clamp (w, h, iw, ih at 0) the derivative is 0; every min / max / clamp is written below as ONE
strict comparison (`lt`, `gt`), and at a tie its derivative goes where that comparison sends the value -- the kernel mirrors
each comparison operand for operand.  Defined for finite inputs only.
"""
import numpy as np

KINDS = {"iou": 0, "giou": 1, "diou": 2}
EPS = 1e-7


def decode(o, anchors, stds):
    """offsets (..., A, 4) -> dict of cx, cy, raw sizes rw / rh, clamped sizes w / h, corners x0, y0, x1, y1 (dtype of o)"""
    ax, ay, aw, ah = (anchors[:, k] for k in range(4))
    cx = o[..., 0] * stds[0] * aw + ax
    cy = o[..., 1] * stds[1] * ah + ay
    ex, ey = np.exp(o[..., 2] * stds[2]), np.exp(o[..., 3] * stds[3])
    rw, rh = (ex - 1) * aw, (ey - 1) * ah
    zero = np.zeros_like(rw)
    w, h = np.where(rw > 0, rw, zero), np.where(rh > 0, rh, zero)
    return dict(cx=cx, cy=cy, ex=ex, ey=ey, rw=rw, rh=rh, w=w, h=h, x0=cx - w / 2, y0=cy - h / 2, x1=cx + w / 2, y1=cy + h / 2)


def smooth_l1(t, p):
    """-> per-anchor smooth-L1 of t - p (sum of the four), d sl1 / d p; oracle.np_ops.localization_loss's expressions"""
    err = t - p
    a = np.abs(err)
    return np.where(a < 1.0, err * err * 0.5, a - 0.5).sum(axis=-1), np.where(a < 1.0, -err, -np.sign(err))


def anchor_terms(t, p, anchors, stds, kind, dtype=np.float64):
    """-> box (B, A), term (B, A), d term / d p (B, A, 4), everything in `dtype`; all anchors, box or not"""
    dt = np.dtype(dtype).type
    t, p, anchors = np.asarray(t, dt), np.asarray(p, dt), np.asarray(anchors, dt)
    stds = [dt(s) for s in stds]
    eps, one, two, half = dt(EPS), dt(1), dt(2), dt(0.5)
    box = ((np.abs(t[..., 0]) + np.abs(t[..., 1]) + np.abs(t[..., 2]) + np.abs(t[..., 3])) > 0).astype(dt)
    g, q = decode(t, anchors, stds), decode(p, anchors, stds)

    def axis(p0, p1, g0, g1):
        """one axis: intersection extent, enclosing extent, and their derivatives w.r.t. the predicted corners p0, p1"""
        hi_lt, lo_gt = p1 < g1, p0 > g0                        # min(p1, g1) = p1 if p1 < g1 else g1; max(p0, g0) = p0 if p0 > g0 else g0
        raw = np.where(hi_lt, p1, g1) - np.where(lo_gt, p0, g0)
        pos = raw > 0
        i = np.where(pos, raw, np.zeros_like(raw))
        hi_gt, lo_lt = p1 > g1, p0 < g0                        # max(p1, g1) = p1 if p1 > g1 else g1; min(p0, g0) = p0 if p0 < g0 else g0
        e = np.where(hi_gt, p1, g1) - np.where(lo_lt, p0, g0)
        return i, e, (pos & hi_lt).astype(dt), (pos & lo_gt).astype(dt), hi_gt.astype(dt), lo_lt.astype(dt)

    iw, ew, diw_1, diw_0, dew_1, dew_0 = axis(q["x0"], q["x1"], g["x0"], g["x1"])      # d iw / d px1 = diw_1, d iw / d px0 = -diw_0
    ih, eh, dih_1, dih_0, deh_1, deh_0 = axis(q["y0"], q["y1"], g["y0"], g["y1"])      # d ew / d px1 = dew_1, d ew / d px0 = -dew_0
    inter = iw * ih
    union = q["w"] * q["h"] + g["w"] * g["h"] - inter
    ue = union + eps
    iou = inter / ue
    term = one - iou
    # gradients of the term w.r.t. I, the predicted area Ap = pw ph, ew, eh, pcx, pcy
    g_i = -(ue + inter) / (ue * ue)
    g_ap = inter / (ue * ue)
    g_ew = g_eh = g_cx = g_cy = np.zeros_like(term)
    if kind == 1:
        enc = ew * eh
        ee = enc + eps
        term = term + (enc - union) / ee
        g_i = g_i + one / ee
        g_ap = g_ap - one / ee
        g_e = ue / (ee * ee)
        g_ew, g_eh = g_e * eh, g_e * ew
    elif kind == 2:
        dx, dy = q["cx"] - g["cx"], q["cy"] - g["cy"]
        rho = dx * dx + dy * dy
        ce = ew * ew + eh * eh + eps
        term = term + rho / ce
        k = -two * rho / (ce * ce)
        g_ew, g_eh = k * ew, k * eh
        g_cx, g_cy = two * dx / ce, two * dy / ce
    else:
        assert kind == 0, kind
    g_iw, g_ih = g_i * ih, g_i * iw
    g_x1 = g_iw * diw_1 + g_ew * dew_1
    g_x0 = -(g_iw * diw_0) - g_ew * dew_0
    g_y1 = g_ih * dih_1 + g_eh * deh_1
    g_y0 = -(g_ih * dih_0) - g_eh * deh_0
    g_w = g_ap * q["h"] + (g_x1 - g_x0) * half
    g_h = g_ap * q["w"] + (g_y1 - g_y0) * half
    aw, ah = anchors[:, 2], anchors[:, 3]
    d = np.stack([(g_cx + g_x0 + g_x1) * (stds[0] * aw),
                  (g_cy + g_y0 + g_y1) * (stds[1] * ah),
                  np.where(q["rw"] > 0, g_w * (stds[2] * aw * q["ex"]), np.zeros_like(g_w)),
                  np.where(q["rh"] > 0, g_h * (stds[3] * ah * q["ey"]), np.zeros_like(g_h))], axis=-1)
    return box, term, d


def iou_localization_loss(t, p, anchors, stds, kind, smooth_l1_weight=1.0, dtype=np.float64):
    """t, p (B, A, 4) offsets, anchors (A, 4) = cx, cy, w, h, stds 4, kind 0 | 1 | 2 (or its name)
    -> loss (B,), d loss_n / d p (B, A, 4) (the per-image normaliser included; exact zeros where box = 0), both in `dtype`"""
    kind = KINDS.get(kind, kind)
    dt = np.dtype(dtype).type
    lam = dt(smooth_l1_weight)
    assert lam >= 0 and np.isfinite(lam)
    t, p = np.asarray(t, dt), np.asarray(p, dt)
    box, term, dterm = anchor_terms(t, p, anchors, stds, kind, dtype)
    sl1, dsl1 = smooth_l1(t, p)
    count = np.maximum(box.sum(axis=-1), dt(1))
    per_anchor = np.where(box > 0, lam * sl1 + term, np.zeros_like(term))
    loss = per_anchor.sum(axis=-1) / count
    d = np.where(box[..., None] > 0, (lam * dsl1 + dterm) / count[:, None, None], np.zeros_like(dterm))
    return loss.astype(dt), d.astype(dt)
