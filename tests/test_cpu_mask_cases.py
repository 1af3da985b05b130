"""The cases, references and bounds of tests/_mask_cases.py, vetted on the CPU alone (no GPU, no library).

The references agree with an independent formulation (torch on the CPU in float64: interpolate, softmax, clamp, log, autograd);
the lattice claims hold (every intermediate of the up-sampling and every partial sum of its transpose is a float32 number); every
named case has the property it is named for, asserted on the float64 reference, so that a changed seed cannot empty it; the clip
decisions are decidable from the reference alone; and every bound is tight enough that each structural error of the issue's list,
applied to the reference, moves it by at least ten times the bound.  Where a case cannot see an error the test names the case and
the reason.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import _mask_cases as MC
import _tail_cases as TC
from oracle import np_ops as O

F32 = np.float32
U = MC.U
POW2_BILINEAR = [s for s in MC.BILINEAR_SHAPES if MC.pow2(s[4]) and MC.pow2(s[5])]
TILE_SHAPES = MC.MASK_X4_SHAPES + MC.MASK_X8_SHAPES


def tag(shape):
    return "x".join(str(s) for s in shape)


def axis_matrix(in_size, out_size, f, align=False, drop=None, tile=None):
    """(out, in) weights of one axis with the geometry restated: f is the factor the source coordinate is formed with (the other
    axis' when the factors are swapped); align: align-corners geometry; drop='first': every input loses the first output of its
    window; tile: every input that ends a tile of `tile` inputs inside the image loses the last output of its window"""
    dst = np.arange(out_size, dtype=np.float64)
    src = dst * (in_size - 1) / max(out_size - 1, 1) if align else (dst + 0.5) / f - 0.5
    src = np.clip(src, 0.0, in_size - 1)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, in_size - 1)
    m = np.zeros((out_size, in_size))
    np.add.at(m, (np.arange(out_size), i0), 1.0 - (src - i0))
    np.add.at(m, (np.arange(out_size), i1), src - i0)
    for i in range(in_size):
        rows = np.flatnonzero(m[:, i])
        if drop == "first":
            m[rows[0], i] = 0.0
        if tile is not None and i % tile == tile - 1 and i != in_size - 1:
            m[rows[-1], i] = 0.0
    return m


def resize(x, my, mx):
    return np.einsum("oh,nhwc,pw->nopc", my, np.asarray(x, np.float64), mx, optimize=True)


def seen(moved, ref, bound, factor=10.0):
    """the error moves some element by at least `factor` times its bound (and by something where the bound is 0)"""
    d = np.abs(np.asarray(moved, np.float64) - ref)
    return bool(((d >= factor * np.broadcast_to(bound, d.shape)) & (d > 0)).any())


# ------------------------------------------------------------------------------------------------- launch mirrors
def test_launch_mirrors():
    n, h, w, fy, fx = MC.MASK_FWD_CAP
    assert h * fy * w * fx == 529984 and MC.partial_blocks(529984) == dict(nblk=256, trips=9)
    assert MC.partial_blocks(524288) == dict(nblk=256, trips=8) and MC.partial_blocks(1)["nblk"] == 1        # the cap binds above 524,288
    n, h, w, fy, fx = MC.MASK_BWD_TRIP
    assert n * h * w == 2099200 and MC.ew_blocks(n * h * w) == dict(blocks=8192, trips=2) and MC.ew_blocks(2097152)["trips"] == 1
    assert MC.partial_blocks(h * w)["trips"] == 17
    assert [MC.mask_bwd_dispatch(*s)[1] for s in MC.MASK_X4_SHAPES] == [1, 4, 4, 1, 3, 8]          # tiles of 16 x 16
    assert [MC.mask_bwd_dispatch(*s)[1] for s in MC.MASK_X8_SHAPES] == [1, 4, 4, 1, 3, 8]          # tiles of 8 x 8
    assert {MC.mask_bwd_dispatch(*s)[0] for s in MC.MASK_X4_SHAPES} == {"(mask_head_bwd_tile_kernel<F, TL>)"}
    assert {MC.mask_bwd_dispatch(*s)[0] for s in MC.MASK_X8_SHAPES} == {"(mask_head_bwd_tile_split_kernel<F, TL, PARTS>)"}
    for s in MC.MASK_GATHER_SHAPES + [MC.MASK_BWD_TRIP]:
        assert MC.mask_bwd_dispatch(*s)[0] == "mask_head_bwd_kernel"
    for s in TILE_SHAPES:
        assert MC.mask_bwd_dispatch(*s, gather=True)[0] == "mask_head_bwd_kernel"
    # h or w of 1, TL - 1, TL and TL + 1 for both tile kernels
    for shapes, tl in ((MC.MASK_X4_SHAPES, MC.TL4), (MC.MASK_X8_SHAPES, MC.TL8)):
        sizes = {s[1] for s in shapes} | {s[2] for s in shapes}
        assert {1, tl - 1, tl, tl + 1} <= sizes
    assert sorted({s[3:] for s in MC.MASK_GATHER_SHAPES}) == [(1, 1), (2, 2), (3, 5), (4, 8), (8, 4), (16, 16)]
    for n, h, w, c, fy, fx in MC.BILINEAR_SHAPES:       # the x4 kernels run only at (4, 4)
        assert MC.bilinear_dispatch(n, h, w, c, fy, fx) == {"bilinear_fwd_kernel": 1}
        assert MC.bilinear_dispatch(n, h, w, c, fy, fx, backward=True) == {"bilinear_bwd_kernel": 1}
    for n, h, w in MC.X4_SHAPES:
        assert MC.bilinear_dispatch(n, h, w, 4, 4, 4) == {"bilinear_fwd_x4_kernel": 1}
        assert MC.bilinear_dispatch(n, h, w, 4, 4, 4, gather=True) == {"bilinear_fwd_kernel": 1}
        want = {"gap_fwd_kernel": 1} if (h, w) == (1, 1) else {"bilinear_bwd_x4_kernel": 1}     # a 1 x 1 backward is the pixel sum
        assert MC.bilinear_dispatch(n, h, w, 4, 4, 4, backward=True) == want
    assert MC.bilinear_dispatch(1, 1, 1, 4, 4, 4, backward=True, accumulate=1) == {"gap_fwd_kernel": 1, "chunk_sum_kernel": 1}
    # partial 2 x 2 blocks of the x4 backward: odd h or w, and h == 1 / w == 1
    assert any(h == 1 and w > 1 for _, h, w in MC.X4_SHAPES) and any(w == 1 and h > 1 for _, h, w in MC.X4_SHAPES)
    assert any(h % 2 and w % 2 and h > 1 for _, h, w in MC.X4_SHAPES)
    assert [c // 4 for c in MC.X4_CHANNELS] == [1, 3, 65]
    n, h, w, c, fy, fx = MC.BILINEAR_FWD_TRIP
    assert MC.ew_blocks(n * h * fy * w * fx * c // 4)["trips"] == 2
    n, h, w, c, fy, fx = MC.BILINEAR_BWD_TRIP
    assert MC.ew_blocks(n * h * w * c // 4)["trips"] == 2


# ------------------------------------------------------------------------------------------------- the lattice
def blend_steps(x, fy, fx, dt):
    """every intermediate of lerp_blend4 in the dtype dt, in the kernel's written order"""
    n, h, w, c = x.shape
    x = x.astype(dt)
    y0, y1, wy = O._bilinear_axis(h, fy, dt)
    x0, x1, wx = O._bilinear_axis(w, fx, dt)
    wx, wy = wx[None, None, :, None], wy[None, :, None, None]
    steps = []

    def lerp(a, b, f):
        d = b - a
        m = d * f
        steps.extend([d, m])
        return a + m
    top = lerp(x[:, y0][:, :, x0], x[:, y0][:, :, x1], wx)
    bot = lerp(x[:, y1][:, :, x0], x[:, y1][:, :, x1], wx)
    out = lerp(top, bot, wy)
    return steps + [top, bot, out]


@pytest.mark.parametrize("mag,offset", [(MC.X_MAG, 0.0), (6.0, 1000.0)])
@pytest.mark.parametrize("fy,fx", [(1, 1), (2, 2), (4, 4), (4, 8), (8, 4), (8, 8), (16, 16)])
def test_lattice_forward_is_exact(fy, fx, mag, offset):
    """every difference, product and sum of the up-sampling of lattice inputs is a float32 number: the float64 reference is what
    the kernel must reproduce bit for bit"""
    x = MC.lattice(MC.seeded(50, fy, fx), (2, 5, 7, 4), mag) + F32(offset)
    for s32, s64 in zip(blend_steps(x, fy, fx, F32), blend_steps(x, fy, fx, np.float64)):
        assert s32.dtype == F32 and np.array_equal(s32.astype(np.float64), s64)
    ref = MC.up(x, fy, fx)
    assert np.array_equal(ref.astype(F32).astype(np.float64), ref) and np.array_equal(ref, blend_steps(x, fy, fx, np.float64)[-1])
    assert not MC.bilinear_fwd_bound(x.astype(np.float64), fy, fx, exact=True).any()


def backward_is_exact(g, h, w, fy, fx, base=None):
    """every weight product is a multiple of 2^-10, every term a multiple of 2^-12, and the absolute terms (and the previous contents)
    sum to less than 2^24 of them: no partial sum of any order rounds"""
    wy, wx = MC.axis_weights(h, fy), MC.axis_weights(w, fx)
    for m in (wy, wx):
        assert np.array_equal(np.round(m * 32), m * 32)
    assert np.array_equal(np.round(g.astype(np.float64) * 4), g.astype(np.float64) * 4)
    total = MC.bilinear_bwd_terms(g, h, w, fy, fx) + (0.0 if base is None else np.abs(base))
    ref = MC.down(g, wy, wx)
    return total.max() < 2.0 ** 24 * 2.0 ** -12 and np.array_equal(ref.astype(F32).astype(np.float64), ref)


def test_lattice_backward_is_exact():
    for n, h, w, c, fy, fx in POW2_BILINEAR + [MC.BILINEAR_FWD_TRIP[:3] + (4, 16, 16)] + [(n, h, w, 4, 4, 4) for n, h, w in MC.X4_SHAPES]:
        g = MC.bilinear_grad(n, h * fy, w * fx, c)
        assert backward_is_exact(g, h, w, fy, fx, MC.bilinear_grad(n, h, w, c)), (n, h, w, c, fy, fx)
        assert not MC.bilinear_bwd_bound(g, h, w, fy, fx, exact=True).any()


# ------------------------------------------------------------------------------------------------- references
def torch_head(case, weights, mode):
    """loss (n,) and d sum(loss) / d logits from torch in float64: mode 'ce' | 'dice' | 'dice_square'"""
    n, h, w, fy, fx = case["shape"]
    z = torch.tensor(case["logits"].astype(np.float64), requires_grad=True)
    upz = TF.interpolate(z.permute(0, 3, 1, 2), size=(h * fy, w * fx), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    p = torch.softmax(upz, -1).reshape(n, -1, 4)
    y = torch.tensor(case["y"].astype(np.float64))
    wt = torch.tensor(TC.w64(weights))
    if mode == "ce":
        loss = -(wt * y * torch.log(torch.clamp(p, MC.LO, MC.HI))).sum((1, 2))
    else:
        inter = (y * p).sum(1)
        total = (y * y + p * p).sum(1) if mode == "dice_square" else (y + p).sum(1)
        loss = (wt * (1 - (2 * inter + TC.KEPS32) / (total + TC.KEPS32))).sum(-1)
    loss.sum().backward()
    return p.detach().numpy(), loss.detach().numpy(), z.grad.numpy()


@pytest.mark.parametrize("shape", MC.MASK_GATHER_SHAPES + [MC.MASK_X4_SHAPES[4]], ids=tag)
def test_references_agree_with_torch(shape):
    """the composed chain O.bilinear_bwd(O.softmax_bwd(...)) and this module's matrix form of it against autograd; the clamp's
    gradient is the `inside` rule away from the bounds, which the decidability rule guarantees"""
    for family in ("clip", "moderate"):
        case = MC.mask_case(shape, family)
        y, p = case["y"], case["p"]
        n, h, w, fy, fx = shape
        tp, tl, tg = torch_head(case, MC.CW, "ce")
        assert np.abs(tp - p).max() < 1e-12
        ref, _ = MC.ce_backward(case, MC.CW, 1.0)
        composed = O.bilinear_bwd(O.softmax_bwd(p, MC.ce_dp(y, p, MC.CW)).reshape(n, h * fy, w * fx, 4), fy, fx)
        scale = np.abs(tg).max()
        assert np.abs(ref - tg).max() <= 1e-12 * scale and np.abs(composed - tg).max() <= 1e-12 * scale
        assert np.abs(MC.ce_ref(y, p, MC.CW) - tl).max() <= 1e-12 * np.abs(tl).max()
        assert np.abs(MC.ce_pixel_ref(y, p, MC.CW).sum(1) - tl).max() <= 1e-12 * np.abs(tl).max()
        for squared, mode in ((0, "dice"), (1, "dice_square")):
            dcase = MC.mask_case(shape, family, "dice")
            _, tl, tg = torch_head(dcase, MC.CW, mode)
            loss, coef = MC.dice_ref(dcase["y"], dcase["p"], MC.CW, squared)
            ref, _ = MC.dice_backward(dcase, MC.CW, squared, 1.0)
            dp = MC.dice_dp(dcase["y"], dcase["p"], coef, squared)
            composed = O.bilinear_bwd(O.softmax_bwd(dcase["p"], dp).reshape(n, h * fy, w * fx, 4), fy, fx)
            scale = np.abs(tg).max()
            assert np.abs(loss - tl).max() <= 1e-12 * np.abs(tl).max()
            assert np.abs(ref - tg).max() <= 1e-12 * scale and np.abs(composed - tg).max() <= 1e-12 * scale


def test_bilinear_references_agree():
    for n, h, w, c, fy, fx in MC.BILINEAR_SHAPES:
        x = MC.bilinear_input(n, h, w, c)
        want = TF.interpolate(torch.tensor(x.astype(np.float64)).permute(0, 3, 1, 2), size=(h * fy, w * fx), mode="bilinear", align_corners=False)
        assert np.abs(MC.up(x, fy, fx) - want.permute(0, 2, 3, 1).numpy()).max() < 1e-12 * MC.X_MAG
        g = MC.bilinear_grad(n, h * fy, w * fx, c)
        mine = MC.down(g, MC.axis_weights(h, fy), MC.axis_weights(w, fx))
        assert np.abs(mine - O.bilinear_bwd(g.astype(np.float64), fy, fx)).max() < 1e-12 * np.abs(mine).max()
        assert np.array_equal(MC.axis_weights(h, fy), axis_matrix(h, h * fy, fy))


# ------------------------------------------------------------------------------------------------- case properties
def test_clip_bounds_are_the_devices():
    assert MC.HI == 1.0 - 2.0 ** -23 and MC.LO == float(F32(1e-7)) and MC.LO != 1e-7 and MC.HI != 1 - 1e-7
    # the band around lo: at p = lo the argument of expf is ln(lo) = -16.1, so a probability carries U (2 x 16.1 + 2) of its own, the
    # p-weighted mean of the row's (the class near 1: 2 U) and 5 U: 41 U; ten of them are 2.5e-5
    z = np.array([[0.0, np.log(MC.LO), -40.0, -40.0]])
    band = MC.DECIDE * TC.softmax_bound(z)[0, 1] / TC.softmax_ref(z)[0, 1]
    assert 2.3e-5 < band < 2.7e-5


@pytest.mark.parametrize("shape", MC.MASK_SHAPES, ids=tag)
def test_mask_cases_have_their_properties(shape):
    n, h, w, fy, fx = shape
    npix = h * fy * w * fx
    families = list(MC.FAMILIES) if shape in MC.MASK_SMALL_SHAPES else ["clip"]
    for family in families:
        case = MC.mask_case(shape, family)
        assert case is not None and case["seed"] < MC.SEEDS                  # a seed without an undecidable entry among the first four
        y, p, bp, logits = case["y"], case["p"], case["bp"], case["logits"]
        assert not MC.undecidable(y, p, bp).any()
        assert np.abs(p.sum(-1) - 1).max() < 1e-12 and (bp > 0).all()
        if family != "normal":
            assert np.array_equal(np.round(logits.astype(np.float64) * 4), logits.astype(np.float64) * 4)
            if MC.pow2(fy) and MC.pow2(fx):                                  # zerr = 0: the logits the softmax sees are exact
                z = MC.up(logits, fy, fx)
                assert np.array_equal(z.astype(F32).astype(np.float64), z) and not MC.logit_error(logits, fy, fx, family).any()
        if family == "clip":
            below, above = MC.clip_sides(y, p)
            assert below >= 0.1 and above >= 0.1, (below, above)
            lab = y != 0
            assert (np.abs(p - MC.LO)[lab] > MC.DECIDE * bp[lab]).all()
        if family == "extreme":                                              # expf underflows to exactly 0 for some classes
            assert (p < 2.0 ** -150).any() and np.abs(logits).max() > 100
        if family == "offset":
            assert logits.min() >= 994 and logits.max() <= 1006
        void, soft = ~y.any(-1), ((y > 0) & (y < 1)).any(-1)
        multi = (y == 1).sum(-1) > 1
        assert void.mean(1).min() >= 0.05
        if npix >= 16:
            assert soft.any() and multi.any() and np.abs(y[soft].sum(-1) - 1).max() == 0
            assert np.array_equal(np.round(y * 8), y * 8)
    dice = MC.mask_case(shape, "clip", "dice")["y"]
    assert not dice[0, :, 3].any() and (~dice.any(-1)).mean(1).min() >= 0.05 and set(np.unique(dice)) <= {0.0, 1.0}
    if n > 1:
        assert not dice[-1].any() and dice[0].any()
    if npix >= 64 and n > 1:
        assert dice[1 if n > 2 else 0].any()


def test_pinned_cases():
    for shape in MC.PINNED_SHAPES:
        for cls, side in ((0, MC.HI), (1, MC.LO)):
            case = MC.pinned_case(shape, cls)
            y, p, bp = case["y"], case["p"], case["bp"]
            assert not MC.undecidable(y, p, bp).any()
            labelled = p[..., cls]
            assert (labelled > MC.HI).all() if cls == 0 else (labelled + bp[..., cls] < MC.LO).all()
            assert (p[..., 0].astype(F32) == 1.0).all()
            ref, _ = MC.ce_backward(case, MC.CW, 0.5)
            assert not ref.any()
            want = y.shape[1] * float(F32(MC.CW[cls])) * -np.log(side)
            assert np.abs(MC.ce_ref(y, p, MC.CW) - want).max() <= 1e-12 * want
            assert (MC.ce_bound(y, p, bp, MC.CW) < 2e-6 * want).all()


# ------------------------------------------------------------------------------------------------- structural errors: bilinear
def wrapped_forward(x, fy, fx):
    """the forward with i1 = i0 + 1 unclamped: the flat index runs into the next row, the next image and, behind the last pixel, the
    NaN that a guarded input is followed by.  lerp_of clamps the source coordinate first, so a clamped output has blend fraction 0
    and the stray element has weight 0: the values cannot see this error, the NaN behind the buffer can (0 x NaN)."""
    n, h, w, c = x.shape
    flat = np.concatenate([x.astype(np.float64).reshape(-1, c), np.full((w + 2, c), np.nan)])
    y0, _, wy = O._bilinear_axis(h, fy, np.float64)
    x0, _, wx = O._bilinear_axis(w, fx, np.float64)
    img = (np.arange(n) * h * w)[:, None, None]
    at = lambda yy, xx: flat[img + yy[None, :, None] * w + xx[None, None, :]]
    wx, wy = wx[None, None, :, None], wy[None, :, None, None]
    top = at(y0, x0) + (at(y0, x0 + 1) - at(y0, x0)) * wx
    bot = at(y0 + 1, x0) + (at(y0 + 1, x0 + 1) - at(y0 + 1, x0)) * wx
    return top + (bot - top) * wy


@pytest.mark.parametrize("n,h,w,c,fy,fx", MC.BILINEAR_SHAPES + [(n, h, w, 4, 4, 4) for n, h, w in MC.X4_SHAPES])
def test_bilinear_bounds_catch_structural_errors(n, h, w, c, fy, fx):
    x = MC.bilinear_input(n, h, w, c).astype(np.float64)
    exact = MC.pow2(fy) and MC.pow2(fx)
    ref, bound = MC.up(x, fy, fx), MC.bilinear_fwd_bound(x, fy, fx, exact=exact)
    assert (bound <= 3e-6 * MC.X_MAG).all()
    my, mx = axis_matrix(h, h * fy, fy), axis_matrix(w, w * fx, fx)
    assert np.abs(resize(x, my, mx) - ref).max() < 1e-12 * MC.X_MAG
    # align-corners geometry.  Blind: a factor of 1 on every axis that has more than one input (both geometries are the identity);
    # an axis of one input has nothing to interpolate
    moving = (h > 1 and fy > 1) or (w > 1 and fx > 1)
    assert seen(resize(x, axis_matrix(h, h * fy, fy, align=True), axis_matrix(w, w * fx, fx, align=True)), ref, bound) == moving
    # fy and fx swapped.  Blind: equal factors; an axis of one input ignores its factor
    swapped = resize(x, axis_matrix(h, h * fy, fx), axis_matrix(w, w * fx, fy))
    assert seen(swapped, ref, bound) == (fy != fx and (h > 1 or w > 1))
    # i1 unclamped: only the NaN behind the buffer shows it (see wrapped_forward); every case has that last pixel
    wrapped = wrapped_forward(x, fy, fx)
    finite = np.isfinite(wrapped)
    assert np.isnan(wrapped[-1, -1, -1]).all() and np.abs(np.where(finite, wrapped - ref, 0.0)).max() < 1e-12 * MC.X_MAG
    # the backward: one window row, and one window column, dropped
    g = MC.bilinear_grad(n, h * fy, w * fx, c)
    bref, bbound = MC.down(g, my, mx), MC.bilinear_bwd_bound(g, h, w, fy, fx, exact)
    assert (bbound <= 1e-4 * max(1.0, np.abs(bref).max())).all()
    assert seen(MC.down(g, axis_matrix(h, h * fy, fy, drop="first"), mx), bref, bbound)
    assert seen(MC.down(g, my, axis_matrix(w, w * fx, fx, drop="first")), bref, bbound)
    if exact:
        assert not bound.any() and not bbound.any()


# ------------------------------------------------------------------------------------------------- structural errors: mask head
def restated(case, my, mx):
    """probabilities of the case's logits under another geometry"""
    n = case["shape"][0]
    return O.softmax(resize(case["logits"], my, mx)).reshape(n, -1, 4)


def backward_with(case, weights, scale, my, mx, **rule):
    n, h, w, fy, fx = case["shape"]
    dz = MC.dz_of(case["p"], MC.ce_dp(case["y"], case["p"], weights, **rule))
    return scale * MC.down(dz.reshape(n, h * fy, w * fx, 4), my, mx)


@pytest.mark.parametrize("shape", MC.MASK_SMALL_SHAPES, ids=tag)
def test_mask_bounds_catch_structural_errors(shape):
    n, h, w, fy, fx = shape
    npix = h * fy * w * fx
    case = MC.mask_case(shape, "clip")
    y, p, bp = case["y"], case["p"], case["bp"]
    my, mx = axis_matrix(h, h * fy, fy), axis_matrix(w, w * fx, fx)
    ref, bound = MC.ce_backward(case, MC.CW, 0.5)
    loss, lbound = MC.ce_ref(y, p, MC.CW), MC.ce_bound(y, p, bp, MC.CW)
    exact = MC.pow2(fy) and MC.pow2(fx)       # (other factors: every logit carries |dsrc| times the steepest step, 60 on this family)
    assert (lbound < 1e-4 * loss).all() and (bound < (1e-3 if exact else 3e-3) * np.abs(ref).max()).all()
    assert np.abs(backward_with(case, MC.CW, 0.5, my, mx) - ref).max() <= 1e-12 * np.abs(ref).max()

    # align-corners geometry, in the probabilities.  Blind: a 1 x 1 source (nothing to interpolate) and a factor of 1
    moving = (h > 1 and fy > 1) or (w > 1 and fx > 1)
    assert seen(restated(case, axis_matrix(h, h * fy, fy, align=True), axis_matrix(w, w * fx, fx, align=True)), p, bp) == moving
    # fy and fx swapped.  Blind: equal factors
    assert seen(restated(case, axis_matrix(h, h * fy, fx), axis_matrix(w, w * fx, fy)), p, bp) == (fy != fx)
    # one window row / column dropped from the backward: on the moderate family, where no gradient row is clipped away (with the
    # clip family a seam that touches eight pixels can meet eight saturated ones)
    dense = MC.mask_case(shape, "moderate")
    dref, dbound = MC.ce_backward(dense, MC.CW, 0.5)
    assert (dbound < (1e-4 if exact else 3e-4) * np.abs(dref).max()).all()
    assert seen(backward_with(dense, MC.CW, 0.5, axis_matrix(h, h * fy, fy, drop="first"), mx), dref, dbound)
    assert seen(backward_with(dense, MC.CW, 0.5, my, axis_matrix(w, w * fx, fx, drop="first")), dref, dbound)
    # a window one output too narrow at a tile seam.  Blind: shapes without a seam inside the image (h and w at most TL) and the
    # gather kernel's shapes, which have no tiles
    if shape in TILE_SHAPES:
        tl = MC.TL4 if fy == 4 else MC.TL8
        narrow = backward_with(dense, MC.CW, 0.5, axis_matrix(h, h * fy, fy, tile=tl), axis_matrix(w, w * fx, fx, tile=tl))
        assert seen(narrow, dref, dbound) == (h > tl or w > tl)
    # the clip rule ignored: no gradient row is zeroed
    assert seen(MC.ce_backward(case, MC.CW, 0.5, clip_rule=False)[0], ref, bound)
    # a void row treated as class 0
    as0 = dict(case, y=np.where(y.any(-1, keepdims=True), y, np.eye(4, dtype=F32)[0]).astype(F32))
    # (the loss always sees it; the gradient unless class 0 is clipped away in every void pixel, as in a 1 x 1 source it can be)
    assert seen(MC.ce_ref(as0["y"], p, MC.CW), loss, lbound)
    assert seen(MC.ce_backward(as0, MC.CW, 0.5)[0], ref, bound) or (h, w) == (1, 1)
    # a partial block of the loss lost or counted twice: every block where there are several; with one block the unit is the image
    terms = MC.ce_pixel_ref(y, p, MC.CW)
    nblk = MC.partial_blocks(npix)["nblk"]
    block = (np.arange(npix) // 256) % nblk
    for q in range(nblk):
        part = terms[:, block == q].sum(1)
        assert (part >= 10 * lbound).all()
    # dice: the same for its sums, through the loss and the coefficients
    dcase = MC.mask_case(shape, "clip", "dice")
    for squared in (0, 1):
        db = MC.dice_bound(dcase["y"], dcase["p"], dcase["bp"], MC.CW, squared)
        assert (db < 1e-4).all()
        if nblk > 1:
            dice_blocks_seen(dcase, squared, nblk)
        # the dice backward: a window row, and a window column, dropped
        dref, dbound = MC.dice_backward(dcase, MC.CW, squared, 0.5)
        ddz = MC.dz_of(dcase["p"], MC.dice_dp(dcase["y"], dcase["p"], MC.dice_ref(dcase["y"], dcase["p"], MC.CW, squared)[1], squared))
        ddz = 0.5 * ddz.reshape(n, h * fy, w * fx, 4)
        assert np.abs(MC.down(ddz, my, mx) - dref).max() <= 1e-12 * np.abs(dref).max()
        assert seen(MC.down(ddz, axis_matrix(h, h * fy, fy, drop="first"), mx), dref, dbound)
        assert seen(MC.down(ddz, my, axis_matrix(w, w * fx, fx, drop="first")), dref, dbound)


def dice_blocks_seen(case, squared, nblk):
    """every partial block of the dice sums, lost: the coefficients A_c = -2 w_c / (T_c + e) of EVERY image move by at least 10 x their
    bound (T is a sum of positive terms); the loss of every image that has labels does too, because the labels agree with the
    probabilities by 256-pixel group (MC.mask_labels) and no block's ratio is the image's.  Blind, in the loss alone: the all-void
    image, whose loss sum w (1 - e / (T + e)) does not depend on the pixels to 1e-7."""
    y, p, bp = case["y"], case["p"], case["bp"]
    n, npix = y.shape[:2]
    block = (np.arange(npix) // 256) % nblk
    y64 = y.astype(np.float64)
    per_block = lambda t: np.stack([[np.bincount(block, weights=t[i, :, k], minlength=nblk) for k in range(4)] for i in range(n)])
    inter, total = MC.dice_sums(y, p, squared)
    ib, tb = per_block(y64 * p), per_block((y64 * y64 + p * p) if squared else (y64 + p))
    w = TC.w64(MC.CW)[None, :, None]
    den = total[:, :, None] - tb + TC.KEPS32
    loss, coef = MC.dice_ref(y, p, MC.CW, squared)
    lost = (w * (1 - (2 * (inter[:, :, None] - ib) + TC.KEPS32) / den)).sum(1)                         # (n, nblk)
    labelled = y.any(axis=(1, 2))
    assert labelled[0] and (np.abs(lost - loss[:, None]) >= 10 * MC.dice_bound(y, p, bp, MC.CW, squared)[:, None])[labelled].all()
    dcoef = MC.SECOND_ORDER * MC.dice_coef_error(y, p, bp, MC.CW, squared)[:, :4, None]
    assert (np.abs(-2 * w / den - coef[:, :4, None]) >= 10 * dcoef).all()


def test_clip_bounds_as_float64_are_seen_by_the_pinned_case():
    """lo: float32(1e-7) and 1e-7 differ by 1e-8 relative, below the 2 ulp of logf; no case can see that, and none needs to.  hi:
    1 - 2^-23 against 1 - 1e-7 moves -log(hi) by 19 %: the pinned above-hi case sees it in the loss.  In the gradient the two upper
    bounds differ only inside the band that hi_term exempts."""
    for shape in MC.PINNED_SHAPES:
        case = MC.pinned_case(shape, 0)
        y, p, bp = case["y"], case["p"], case["bp"]
        assert seen(MC.ce_ref(y, p, MC.CW, lo=1e-7, hi=1 - 1e-7), MC.ce_ref(y, p, MC.CW), MC.ce_bound(y, p, bp, MC.CW))
    case = MC.mask_case(MC.MASK_X4_SHAPES[5], "clip")
    y, p, bp = case["y"], case["p"], case["bp"]
    assert not seen(MC.ce_ref(y, p, MC.CW, lo=1e-7, hi=1 - 1e-7), MC.ce_ref(y, p, MC.CW), MC.ce_bound(y, p, bp, MC.CW))
    ref, bound = MC.ce_backward(case, MC.CW, 0.5)
    assert not seen(MC.ce_backward(case, MC.CW, 0.5, lo=1e-7, hi=1 - 1e-7)[0], ref, bound, factor=1.0)


def test_capped_grid_cases_see_a_lost_block():
    """the ninth trip and the second grid-stride trip: every one of the 256 blocks, lost, moves the loss by 10 x the bound; the
    pixels of the second trip of the gather backward, lost, move dlogits"""
    for shape in (MC.MASK_FWD_CAP, MC.MASK_BWD_TRIP):
        case = MC.mask_case(shape, "clip")
        y, p, bp = case["y"], case["p"], case["bp"]
        npix = y.shape[1]
        la = MC.partial_blocks(npix)
        assert la["nblk"] == 256 and la["trips"] >= 9
        terms = MC.ce_pixel_ref(y, p, MC.CW)
        lbound = MC.ce_bound(y, p, bp, MC.CW)
        block = (np.arange(npix) // 256) % 256
        parts = np.stack([np.bincount(block, weights=t, minlength=256) for t in terms])
        assert (parts >= 10 * lbound[:, None]).all()
        ninth = terms[:, 8 * 65536:].sum(1)                                  # what the threads add on their ninth trip and later
        assert (ninth >= 10 * lbound).all()
        dcase = MC.mask_case(shape, "clip", "dice")                          # the dice kernel's 256 partial rows of eight sums
        assert dcase is not None
        for squared in (0, 1):
            dice_blocks_seen(dcase, squared, 256)
    n, h, w, fy, fx = MC.MASK_BWD_TRIP
    ref, bound = MC.ce_backward(case, MC.CW_ONE, 1.0)
    second = ref.reshape(-1, 4)[MC.EW_CAP * 256:]
    assert second.shape[0] == n * h * w - 2097152 and (np.abs(second) >= 10 * bound.reshape(-1, 4)[MC.EW_CAP * 256:]).any()


def test_weights_and_loss_scales_meet_in_every_pair():
    for shapes in (MC.MASK_X4_SHAPES, MC.MASK_X8_SHAPES, MC.MASK_GATHER_SHAPES):
        pairs = {(MC.mask_settings(s, k)[0], MC.LOSS_SCALES.index(None if v == 1.0 / s[0] and v != 0.5 else v))
                 for s in shapes for k in range(len(MC.FAMILIES)) for v in [MC.mask_settings(s, k)[1]]}
        assert len(pairs) == 9


def test_hi_term_against_the_plain_absolute_term():
    """hi_term is the larger of 2^-22 w_c y_c and the reference's share w_c y_c (1 - p_c), 1 - p_c <= 2^-23 + upward_error <= 7 U (1 + rho).
    The largest hi_term / (2^-22 w_c y_c) over every case and family is printed (DESIGN.md records it): never more than 1.77 (1 + rho), second-order factor included"""
    worst = {}
    for shape in MC.MASK_SHAPES:
        for family in (MC.FAMILIES if shape in MC.MASK_SMALL_SHAPES else ["clip"]):
            case = MC.mask_case(shape, family)
            y, p, bp = case["y"], case["p"], case["bp"]
            flag = (y != 0) & (p + MC.upward_error(p, bp) >= MC.HI)
            plain = 2.0 ** -22 * (flag * np.abs(TC.w64(MC.CW) * y)).sum(-1, keepdims=True)
            term = MC.hi_term(y, p, bp, MC.CW)
            assert not term[~flag.any(-1)].any()
            if flag.any():
                rows = flag.any(-1)
                widening = float((term[rows] / plain[rows]).max())
                assert 1.0 <= widening <= 1.77 * (1 + float((bp / np.maximum(p, 1e-30) * (p >= 1e-30)).max()))
                worst[(shape, family)] = widening
    assert worst
    for name, keys in (("power-of-two factors", [k for k in worst if MC.pow2(k[0][3]) and MC.pow2(k[0][4])]),
                       ("other factors", [k for k in worst if not (MC.pow2(k[0][3]) and MC.pow2(k[0][4]))])):
        top = max(keys, key=worst.get)
        print(f"\nlargest hi_term / (2^-22 w y), {name}: {worst[top]:.3g} at {top}; flagged cases: {len(keys)}")
