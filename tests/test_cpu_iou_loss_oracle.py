"""The IoU-family box regression loss without a GPU: the public factory's surface; the NumPy spec (tests/_iou_loss_oracle.py) pinned
against the same loss written in torch (CPU autograd, float64), against central differences and on hand-worked boxes; and the
shared inputs of the GPU test (tests/_iou_loss_cases.py): clear of every kink, and what float32 costs on them.
test_gpu_iou_loss.py then pins the kernel to the spec."""
import numpy as np
import pytest

import _iou_loss_cases as K
import _iou_loss_oracle as S

KINDS = [0, 1, 2]
ANCHOR = np.array([[100.0, 80.0, 40.0, 20.0]])          # one default box: centre (100, 80), 40 x 20
STDS = K.STDS


def rel_err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def encode(cx, cy, w, h, anchor=ANCHOR[0]):
    """the offsets that decode to the box (cx, cy, w, h) against `anchor`"""
    ax, ay, aw, ah = anchor
    return [(cx - ax) / (STDS[0] * aw), (cy - ay) / (STDS[1] * ah), np.log1p(w / aw) / STDS[2], np.log1p(h / ah) / STDS[3]]


# -------------------------------------------------------------------------------------------------------------- the surface
def test_factory_surface():
    import ssdseglib
    d = np.arange(1, 7, dtype=np.float32)
    fn = ssdseglib.losses.iou_localization_loss(d, d, d, d, STDS)
    assert fn.__name__ == "iou_localization_loss" and fn.loss_kind == "iou_loc" and callable(fn)
    assert fn.kind == "giou" and fn.smooth_l1_weight == 1.0 and type(fn.smooth_l1_weight) is float
    assert callable(fn.anchors_on) and fn.n_anchors == 6
    for kind in ("iou", "giou", "diou"):
        fn = ssdseglib.losses.iou_localization_loss(list(d), d, d.reshape(2, 3), d, [0.1, 0.1, 0.2, 0.2], kind=kind, smooth_l1_weight=0)
        assert fn.kind == kind and fn.smooth_l1_weight == 0.0 and fn.n_anchors == 6
    assert ssdseglib.losses.IOU_KINDS == S.KINDS


D6 = np.ones(6, np.float32)


@pytest.mark.parametrize("kwargs", [dict(kind="ciou"), dict(kind=1), dict(kind=None), dict(smooth_l1_weight=-0.5),
                                    dict(smooth_l1_weight=float("nan")), dict(smooth_l1_weight=float("inf")), dict(smooth_l1_weight="x"),
                                    dict(stds=(0.1, 0.1, 0.2)), dict(stds=(0.1,) * 5), dict(stds=(0.1, 0.0, 0.2, 0.2)),
                                    dict(stds=(0.1, -0.1, 0.2, 0.2)), dict(stds=(0.1, float("inf"), 0.2, 0.2)),
                                    dict(stds=(0.1, float("nan"), 0.2, 0.2)), dict(stds=0.1), dict(w=np.ones(5, np.float32)),
                                    dict(cx=np.ones(7, np.float32)), dict(cx=np.ones(0), cy=np.ones(0), w=np.ones(0), h=np.ones(0))])
def test_factory_rejects_bad_arguments_without_a_device(kwargs, monkeypatch):
    import ssdseglib
    from ssdseglib import _engine

    def no_device():
        raise AssertionError("the factory touched the GPU")
    monkeypatch.setattr(_engine, "default_context", no_device)
    kw = dict(kwargs)
    args = [kw.pop(k, D6) for k in ("cx", "cy", "w", "h")] + [kw.pop("stds", STDS)]
    with pytest.raises(ValueError):
        ssdseglib.losses.iou_localization_loss(*args, **kw)
    ssdseglib.losses.iou_localization_loss(D6, D6, D6, D6, (1e-3, 0.1, 0.2, 5.0), kind="iou", smooth_l1_weight=0.0)     # edges of the valid range


# ------------------------------------------------------------------------------------------------ the spec against torch
def small_case(which, seed=17, b=3, a=40, pos_frac=0.3):
    """float64 copies of a small case of the shared builder, image 1 without objects; asserted tie-free"""
    t, p, an = K.make_case(seed, b, a, pos_frac, which)
    t, p, an = t.astype(np.float64), p.astype(np.float64), an.astype(np.float64)
    t[1] = 0.0
    px, knee = K.kink_margins(t, p, an)
    assert px > K.MARGIN_PX and knee > K.MARGIN_KNEE, (px, knee)
    return t, p, an


def torch_loss(t, p, an, kind, lam):
    import torch
    tt, tan = torch.tensor(t, dtype=torch.float64), torch.tensor(an, dtype=torch.float64)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    s = STDS

    def dec(o):
        cx, cy = o[..., 0] * s[0] * tan[:, 2] + tan[:, 0], o[..., 1] * s[1] * tan[:, 3] + tan[:, 1]
        w = torch.clamp((torch.exp(o[..., 2] * s[2]) - 1) * tan[:, 2], min=0)
        h = torch.clamp((torch.exp(o[..., 3] * s[3]) - 1) * tan[:, 3], min=0)
        return cx, cy, w, h, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2

    gcx, gcy, gw, gh, gx0, gy0, gx1, gy1 = dec(tt)
    pcx, pcy, pw, ph, px0, py0, px1, py1 = dec(tp)
    iw = torch.clamp(torch.minimum(px1, gx1) - torch.maximum(px0, gx0), min=0)
    ih = torch.clamp(torch.minimum(py1, gy1) - torch.maximum(py0, gy0), min=0)
    inter = iw * ih
    union = pw * ph + gw * gh - inter
    ew, eh = torch.maximum(px1, gx1) - torch.minimum(px0, gx0), torch.maximum(py1, gy1) - torch.minimum(py0, gy0)
    term = 1 - inter / (union + 1e-7)
    if kind == 1:
        term = term + (ew * eh - union) / (ew * eh + 1e-7)
    elif kind == 2:
        term = term + ((pcx - gcx) ** 2 + (pcy - gcy) ** 2) / (ew ** 2 + eh ** 2 + 1e-7)
    err = tt - tp
    sl1 = torch.where(err.abs() < 1, 0.5 * err * err, err.abs() - 0.5).sum(-1)
    box = (tt.abs().sum(-1) > 0).to(torch.float64)
    loss = (box * (lam * sl1 + term)).sum(-1) / torch.clamp(box.sum(-1), min=1.0)
    loss.sum().backward()
    return loss.detach().numpy(), tp.grad.numpy()


@pytest.mark.parametrize("which", K.SETS)
@pytest.mark.parametrize("lam", K.LAMBDAS)
@pytest.mark.parametrize("kind", KINDS)
def test_value_and_gradient_against_torch_autograd(kind, lam, which):
    t, p, an = small_case(which)
    loss, d = S.iou_localization_loss(t, p, an, STDS, kind, lam)
    tl, td = torch_loss(t, p, an, kind, lam)
    assert loss[1] == 0 and not d[1].any()                      # the image without objects: 0 / max(0, 1)
    assert loss[0] > 0 and np.abs(d[0]).max() > 0
    assert rel_err(loss, tl) < 1e-12
    assert rel_err(d, td) < 1e-12
    assert not d[np.abs(t).sum(-1) == 0].any()


@pytest.mark.parametrize("which", K.SETS)
@pytest.mark.parametrize("lam", K.LAMBDAS)
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_against_central_differences(kind, lam, which):
    """h = 1e-6 in offset units moves a corner by at most 1e-6 * 0.2 * 671 * e^(0.2 * 8) < 1e-3 px, so no branch changes inside
    the stencil; rounding 1e-16 |loss| / h ~ 1e-10 and truncation h^2 f''' / 6 ~ 1e-12 f''' against gradients of order 0.01 .. 1:
    inside 1e-6 of the largest gradient"""
    t, p, an = small_case(which, b=2, a=12, pos_frac=0.5)
    _, d = S.iou_localization_loss(t, p, an, STDS, kind, lam)
    h = 1e-6
    fd = np.zeros_like(d)
    for idx in np.ndindex(*p.shape):
        up, dn = p.copy(), p.copy()
        up[idx] += h
        dn[idx] -= h
        lu, _ = S.iou_localization_loss(t, up, an, STDS, kind, lam)
        ld, _ = S.iou_localization_loss(t, dn, an, STDS, kind, lam)
        fd[idx] = (lu[idx[0]] - ld[idx[0]]) / (2 * h)
        other = [i for i in range(p.shape[0]) if i != idx[0]]
        assert np.array_equal(lu[other], ld[other])             # no image depends on another one
    assert np.abs(d).max() > 1e-3
    assert np.abs(d - fd).max() < 1e-6 * np.abs(d).max()


# ------------------------------------------------------------------------------------------------------- hand-worked cases
@pytest.mark.parametrize("kind", KINDS)
def test_identical_boxes(kind):
    """p = t: IoU = A / (A + 1e-7), the enclosing box is the box, the centres coincide -- the GIoU and DIoU penalties are 0 and every
    term is 1 - IoU = 1e-7 / (A + 1e-7)"""
    t = np.array([[encode(110.0, 85.0, 30.0, 16.0)]])
    loss, d = S.iou_localization_loss(t, t.copy(), ANCHOR, STDS, kind, 1.0)
    assert abs(loss[0] - 1e-7 / (480.0 + 1e-7)) < 1e-15
    # every min / max is a tie and sends the value to the target's corner: no gradient through the intersection or the
    # enclosing box, only through the predicted area in U
    assert d[0, 0, 0] == 0 and d[0, 0, 1] == 0


def test_disjoint_boxes():
    """target 30 x 16 at (110, 85), prediction 10 x 8 at (160, 120): no overlap.  IoU term exactly 1 with a zero gradient; GIoU
    = 1 + (E - U) / E with E = (165 - 95) (124 - 77) = 3290, U = 480 + 80, and a gradient that pulls the prediction in"""
    t = np.array([[encode(110.0, 85.0, 30.0, 16.0)]])
    p = np.array([[encode(160.0, 120.0, 10.0, 8.0)]])
    loss, d = S.iou_localization_loss(t, p, ANCHOR, STDS, 0, 0.0)
    assert loss[0] == 1.0 and not d.any()
    loss, d = S.iou_localization_loss(t, p, ANCHOR, STDS, 1, 0.0)
    assert abs(loss[0] - (1.0 + (3290.0 - 560.0) / (3290.0 + 1e-7))) < 1e-12
    assert d[0, 0, 0] > 0 and d[0, 0, 1] > 0                    # moving the centre further right / down raises the loss
    loss, d = S.iou_localization_loss(t, p, ANCHOR, STDS, 2, 0.0)
    assert abs(loss[0] - (1.0 + (50.0 ** 2 + 35.0 ** 2) / (70.0 ** 2 + 47.0 ** 2 + 1e-7))) < 1e-12
    assert d[0, 0, 0] > 0 and d[0, 0, 1] > 0
    _, dl = S.iou_localization_loss(t, p, ANCHOR, STDS, 0, 1.0)
    _, dsl1 = S.smooth_l1(t, p)
    assert np.array_equal(dl, dsl1)                             # with the IoU kind only smooth-L1 moves a disjoint box


@pytest.mark.parametrize("kind", KINDS)
def test_raw_size_at_or_below_zero_has_no_size_gradient(kind):
    """an untrained head: size offsets 0 (raw size exactly 0) and below.  With smooth_l1_weight = 0 the size components of the
    gradient are exactly 0 -- the reason smooth-L1 stays in the loss; with weight 1 they are smooth-L1's"""
    t = np.array([[encode(104.0, 82.0, 30.0, 16.0)] * 3])
    p = np.array([[[0.1, -0.2, 0.0, 0.0], [0.1, -0.2, -0.5, 0.0], [0.1, -0.2, 0.0, -2.0]]])
    an = np.repeat(ANCHOR, 3, axis=0)
    loss, d = S.iou_localization_loss(t, p, an, STDS, kind, 0.0)
    assert np.isfinite(loss).all() and not d[..., 2:].any()
    _, d1 = S.iou_localization_loss(t, p, an, STDS, kind, 1.0)
    _, dsl1 = S.smooth_l1(t, p)
    assert np.array_equal(d1[..., 2:], dsl1[..., 2:] / 3.0) and d1[..., 2:].all()
    # one positive size is not enough either: the area pw ph and the intersection stay 0 while the other size is clamped
    p2 = np.array([[[0.1, -0.2, 1.0, 0.0]] * 3])
    _, d2 = S.iou_localization_loss(t, p2, an, STDS, 0, 0.0)
    assert not d2.any()


# --------------------------------------------------------------------------------------------- the GPU test's shared inputs
ALL_CASES = [(sh, which) for sh in K.SHAPES for which in K.SETS]


@pytest.mark.parametrize("shape,which", ALL_CASES)
def test_shared_cases_keep_clear_of_every_kink(shape, which):
    """every box-carrying anchor: operands of each min / max / clamp more than 1e-3 px apart, | |t - p| - 1 | > 1e-4.  float32
    and float64 then take the same branch everywhere, and the share of anchors left out of the GPU comparison is 0"""
    b, a, pos_frac = shape
    t, p, an = K.case(b, a, pos_frac, which)
    assert t.dtype == p.dtype == an.dtype == np.float32 and t.shape == p.shape == (b, a, 4) and an.shape == (a, 4)
    box = np.abs(t).sum(-1) > 0
    assert (box.sum() == 0) == (pos_frac == 0.0)
    if pos_frac > 0:
        assert box.sum(-1).min() >= 1
        g = S.decode(t.astype(np.float64), an.astype(np.float64), STDS)
        assert g["rw"][box].min() > 0 and g["rh"][box].min() > 0          # targets with positive sizes
        q = S.decode(p.astype(np.float64), an.astype(np.float64), STDS)
        clamped = (q["rw"][box] <= 0).mean()
        if which == "near":
            assert clamped < 0.1
        elif box.sum() > 20:
            assert 0.3 < clamped < 0.7                                      # an untrained head: either sign
    px, knee = K.kink_margins(t, p, an)
    assert px > K.MARGIN_PX and knee > K.MARGIN_KNEE, (px, knee)
    if a == 9600:
        assert np.array_equal(an, K.all_default_boxes())


def f32_errors(t, p, an, kind, lam):
    l64, d64 = S.iou_localization_loss(t, p, an, STDS, kind, lam)
    l32, d32 = S.iou_localization_loss(t, p, an, STDS, kind, lam, dtype=np.float32)
    assert l32.dtype == np.float32 and d32.dtype == np.float32
    if not np.abs(l64).max() > 0:
        assert not l32.any() and not d32.any() and not d64.any()
        return 0.0, 0.0
    return float(rel_err(l32, l64)), float(np.abs(d32 - d64).max() / np.abs(d64).max())


def test_float32_numpy_error_of_the_spec_on_the_shared_cases():
    """what single precision alone costs on the GPU test's inputs: the recorded worst errors (K.F32_LOSS_REL, K.F32_DBOX_ABS, the
    basis of the GPU bounds) are the measured ones.  NumPy's float32 exp differs in the last bit between its SIMD paths, so the
    measurement may sit a little off the record: within [0.5, 1.25] x of it."""
    inputs = [K.case(*sh, which) for sh, which in ALL_CASES] + [K.tie_case()[:3]]
    worst_loss = worst_d = 0.0
    for t, p, an in inputs:
        for kind in KINDS:
            for lam in K.LAMBDAS:
                el, ed = f32_errors(t, p, an, kind, lam)
                worst_loss, worst_d = max(worst_loss, el), max(worst_d, ed)
    print(f"float32 NumPy against float64: loss rel {worst_loss:.3e}, d_boxes abs / max {worst_d:.3e}")
    assert 0.5 * K.F32_LOSS_REL <= worst_loss <= 1.25 * K.F32_LOSS_REL
    assert 0.5 * K.F32_DBOX_ABS <= worst_d <= 1.25 * K.F32_DBOX_ABS


def test_tie_and_clamp_cases_are_what_they_say():
    t, p, an, rows = K.tie_case()
    assert rows.shape[0] > 100 and np.array_equal(p[rows[:, 0], rows[:, 1]].view(np.uint32), t[rows[:, 0], rows[:, 1]].view(np.uint32))
    t, p, an = K.clamp_case()
    box = np.abs(t).sum(-1) > 0
    q = S.decode(p.astype(np.float64), an.astype(np.float64), STDS)
    assert ((q["rw"] <= 0) & box).sum() > 10 and ((q["rh"] <= 0) & box).sum() > 10
    for kind in KINDS:
        _, d = S.iou_localization_loss(t, p, an, STDS, kind, 0.0)
        assert not d[..., 2][q["rw"] <= 0].any() and not d[..., 3][q["rh"] <= 0].any()
