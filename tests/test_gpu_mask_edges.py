"""GPU parity of the bilinear resize and the mask head at their edges (through the C-ABI) vs float64.

ssdseg_bilinear_fwd / _fwd_padded / _bwd (csrc/resize.hip) and ssdseg_mask_head_fwd / _bwd / _fwd_dice / _bwd_dice / _fwd_bootstrap /
_bwd_bootstrap (csrc/mask_head.hip) on the cases of tests/_mask_cases.py: sources of one row, one column and one pixel, tiles of TL
and TL +- 1 pixels for both tile kernels, every factor pair of the gather kernels, factors that are no power of two, the capped
grids (a thread's ninth pixel and more, a second grid-stride trip), logits that drive probabilities to both sides of the clip
interval and into underflow, labels that are void, soft or multi-hot, zero weights, loss scales 0 and below, every activation code
of the bilinear view, row pitches with gaps and channel slices, and the argument contracts.  tests/test_cpu_mask_cases.py vets the
references, the cases and the bounds.  Every buffer is guarded (tests/_guard.py); every launch is read from the timing registry.

The bounds are derived, not tuned; the derivations stand with the functions in tests/_mask_cases.py.  U = 2^-24.

  bilinear, lattice input, power-of-two factors, plain view   exact (bound 0), forward and backward, general and x4, padded or not
  bilinear, other factors     |dsrc| <= 3 U (dst + 0.5) / f per axis times the steepest step of the input, + the roundings of lerp_blend4;
                              backward: the same |dsrc| on every weight, + gamma(window) of the absolute terms
  bilinear, affine view       + 1 ULP of |s x| + |t| per corner
  probabilities               TC.softmax_bound (zerr = 0 on the lattice); row sums within 4 U of 1
  losses                      per term bp / p on log p and 2 ulp of logf, then gamma(trips + 8 + roundings of a term); dice through r
  dlogits                     per pixel absolute on p_c (|dp_c| + |dot|), summed over the window with |wy wx loss_scale|, + gamma(window),
                              + the upper clip bound's 2^-22 w_c |loss_scale| per contributing pixel
  zero weights, void images, loss_scale 0                      exact zeros

Run with -s for the largest error / bound ratio of every case (DESIGN.md records them).
"""
import numpy as np
import pytest

import _mask_cases as MC
import _tail_cases as TC
from oracle import np_ops as O
from _guard import BODY_WORD, INPUT_WORD, guards  # noqa: F401  (fixture)
from _edge_helpers import c4, dev_view, finish, launched, ratio, rejected, reporter, same_bits, untouched

pytestmark = pytest.mark.gpu

F32 = np.float32
U = MC.U
FORMS = ("dense", "pitched", "slice")
FWD_KERNELS = {"mask_head_fwd_kernel": 1, "mask_loss_final_kernel": 1}
DICE_KERNELS = {"mask_head_fwd_dice_kernel": 1, "mask_dice_final_kernel": 1}


report = reporter("mask-edges")


def tag(shape):
    return "x".join(str(s) for s in shape)


# ------------------------------------------------------------------------------------------------------ operand forms
def operand_in(guards, a, c, form):
    """a (rows, c) as an input: dense | pitched (ld = c + 4, NaN gaps) | slice (columns 4 .. 4 + c of a c + 8 wide buffer of NaNs)
    -> (what the call takes, ld)"""
    a = np.ascontiguousarray(a, F32).reshape(-1, c)
    if form == "dense":
        return guards.inp(a), c
    if form == "pitched":
        return guards.inp(a, ld=c + 4), c + 4
    wide = np.full((a.shape[0], c + 8), INPUT_WORD, np.uint32).view(F32)
    wide[:, 4:4 + c] = a
    buf = guards.inp(wide)
    return buf.view(4, (buf.size - 4,)), c + 8


def operand_out(guards, rows, c, form, base=None):
    """an output of (rows, c) in the same three forms, holding `base` (accumulate) or poison -> (what the call takes, ld, read);
    read() returns the (rows, c) result and asserts that the columns around a slice are bit-unchanged"""
    if form != "slice":
        ld = c if form == "dense" else c + 8
        buf = guards.out((rows, c), ld=ld)
        if base is not None:
            buf.upload(base.reshape(rows, c))
        return buf, ld, buf.download
    wide = guards.out((rows, c + 8))
    if base is not None:
        w0 = np.full((rows, c + 8), BODY_WORD, np.uint32).view(F32)
        w0[:, 4:4 + c] = base.reshape(rows, c)
        wide.upload(w0)

    def read():
        got = wide.download()
        assert (got[:, :4].view(np.uint32) == BODY_WORD).all() and (got[:, 4 + c:].view(np.uint32) == BODY_WORD).all()
        return got[:, 4:4 + c].copy()
    return wide.view(4, (wide.size - 4,)), c + 8, read


def poisoned(a):
    return int((np.ascontiguousarray(a).view(np.uint32) == np.uint32(BODY_WORD)).sum())


# ------------------------------------------------------------------------------------------------------------ bilinear
def bilinear_fwd(ctx, guards, x, s, t, act, fy, fx, form, expect):
    from ssdseglib import _hip as H
    n, h, w, c = x.shape
    xb, ldx = operand_in(guards, x, c, form)
    view = H.view(xb, act=act) if s is None else H.view(xb, guards.inp(s), guards.inp(t), act)
    out, ldo, read = operand_out(guards, n * h * fy * w * fx, c, form)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_bilinear_fwd", view, ldx, out, ldo, n, h, w, c, fy, fx))
    assert kernels == expect, (kernels, expect)
    got = read().reshape(n, h * fy, w * fx, c)
    assert poisoned(got) == 0
    return got


def bilinear_bwd(ctx, guards, g, h, w, fy, fx, accumulate, form, expect, base=None):
    n, c = g.shape[0], g.shape[3]
    gb, ldg = operand_in(guards, g, c, form)
    dx, ldx, read = operand_out(guards, n * h * w, c, form, base if accumulate else None)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_bilinear_bwd", gb, ldg, dx, ldx, n, h, w, c, fy, fx, accumulate))
    assert kernels == expect, (kernels, expect)
    got = read().reshape(n, h, w, c)
    assert poisoned(got) == 0
    return got


def bilinear_case(ctx, guards, monkeypatch, n, h, w, c, fy, fx, gather=False):
    """the forward with a plain and an affine view under each activation code, the backward with and without accumulate, every
    operand form; -> the ratios and the results (for the bit-identity claims)"""
    if gather:
        monkeypatch.setenv("SSDSEG_BILINEAR", "gather")
    x = MC.bilinear_input(n, h, w, c)
    exact = MC.pow2(fy) and MC.pow2(fx)
    s, t = TC.view_params(c, 9)
    ratios, results, k = {}, {}, 0
    expect = MC.bilinear_dispatch(n, h, w, c, fy, fx, gather=gather)
    for affine in (False, True):
        for act in TC.ACTS:
            a, mag = TC.view_ref(x, s if affine else None, t if affine else None, act)
            got = bilinear_fwd(ctx, guards, x, s if affine else None, t if affine else None, act, fy, fx, FORMS[k % 3], expect)
            bound = MC.bilinear_fwd_bound(a, fy, fx, mag if affine else None, exact=exact and not affine)
            name = f"fwd-{'affine' if affine else 'plain'}-{TC.ACT_NAMES[act]}"
            ratios[name] = ratio(got, MC.up(a, fy, fx), bound)
            results[name] = got
            k += 1
    g = MC.bilinear_grad(n, h * fy, w * fx, c)
    base = MC.bilinear_grad(n, h, w, c)
    ref = MC.down(g, MC.axis_weights(h, fy), MC.axis_weights(w, fx))
    for accumulate in (0, 1):
        for form in FORMS:
            pitched = form != "dense"
            expect_b = MC.bilinear_dispatch(n, h, w, c, fy, fx, True, accumulate, pitched, gather)
            got = bilinear_bwd(ctx, guards, g, h, w, fy, fx, accumulate, form, expect_b, base)
            want = ref + (base if accumulate else 0.0)
            if h == 1 and w == 1:       # the pixel sum: exact on the lattice like the others
                bound = np.zeros(want.shape)
            else:                       # the addition to the previous contents is one rounding unless the sum is exact
                bound = MC.bilinear_bwd_bound(g, h, w, fy, fx, exact) + (0.0 if exact or not accumulate else U * np.abs(want))
            name = f"bwd-acc{accumulate}-{form}"
            ratios[name] = ratio(got, want, bound)
            results[name] = got
    if gather:
        monkeypatch.delenv("SSDSEG_BILINEAR")
    return ratios, results


@pytest.mark.parametrize("n,h,w,c,fy,fx", MC.BILINEAR_SHAPES)
def test_bilinear_general_edges(ctx, guards, monkeypatch, n, h, w, c, fy, fx):
    ratios, _ = bilinear_case(ctx, guards, monkeypatch, n, h, w, c, fy, fx)
    if MC.pow2(fy) and MC.pow2(fx):
        assert not any(v for k, v in ratios.items() if "affine" not in k)       # exact
    report("bilinear", f"{tag((n, h, w, c))} x{fy}x{fx}", **ratios)
    finish(ctx, guards)


@pytest.mark.parametrize("c", MC.X4_CHANNELS)
@pytest.mark.parametrize("n,h,w", MC.X4_SHAPES)
def test_bilinear_x4_edges(ctx, guards, monkeypatch, n, h, w, c):
    """the x4 kernels against float64 (exact on the lattice) and against the general kernels under SSDSEG_BILINEAR=gather: the
    forward bit-identical with every view, the backward bit-identical because both are exact; a 1 x 1 source's backward is the pixel
    sum either way"""
    ratios, x4 = bilinear_case(ctx, guards, monkeypatch, n, h, w, c, 4, 4)
    _, general = bilinear_case(ctx, guards, monkeypatch, n, h, w, c, 4, 4, gather=True)
    for name in x4:
        assert same_bits(x4[name], general[name]), name
    assert not any(v for k, v in ratios.items() if "affine" not in k)
    report("bilinear x4", f"{tag((n, h, w, c))}", **ratios)
    finish(ctx, guards)


@pytest.mark.parametrize("affine", (False, True), ids=("plain", "affine+relu6"))
@pytest.mark.parametrize("fy,fx", MC.PADDED_FACTORS)
def test_bilinear_fwd_padded_edges(ctx, guards, fy, fx, affine):
    """the interior of the bordered tensor == the plain forward bit for bit; the border keeps its poison, the gap columns their
    guard word (guards.check)"""
    n, h, w, c, ldo = 2, 3, 5, 8, 12
    x = MC.bilinear_input(n, h, w, c)
    s, t, act = (*TC.view_params(c, 9), O.ACT_RELU6) if affine else (None, None, O.ACT_NONE)
    view = dev_view(guards, x, s, t, act)
    plain = guards.out((n, h * fy, w * fx, c))
    ctx.call("ssdseg_bilinear_fwd", view, c, plain, c, n, h, w, c, fy, fx)
    padded = guards.out((n, h * fy + 2, w * fx + 2, c), ld=ldo)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_bilinear_fwd_padded", view, c, padded, ldo, n, h, w, c, fy, fx))
    assert kernels == MC.bilinear_dispatch(n, h, w, c, fy, fx)
    got = padded.download()
    assert same_bits(got[:, 1:-1, 1:-1], plain.download())
    border = np.ones(got.shape[:3], bool)
    border[:, 1:-1, 1:-1] = False
    assert (got.view(np.uint32)[border] == np.uint32(BODY_WORD)).all() and poisoned(got[:, 1:-1, 1:-1]) == 0
    a, mag = TC.view_ref(x, s, t, act)
    exact = MC.pow2(fy) and MC.pow2(fx) and not affine
    report("bilinear padded", f"x{fy}x{fx} {'affine' if affine else 'plain'}",
           out=ratio(got[:, 1:-1, 1:-1], MC.up(a, fy, fx), MC.bilinear_fwd_bound(a, fy, fx, mag if affine else None, exact=exact)))
    finish(ctx, guards)


def test_bilinear_second_trips(ctx, guards):
    """more than 8192 x 256 threads in the general kernels: the forward at x16, the backward at x1 (the identity)"""
    n, h, w, c, fy, fx = MC.BILINEAR_FWD_TRIP
    assert MC.ew_blocks(n * h * fy * w * fx * c // 4)["trips"] == 2
    x = MC.bilinear_input(n, h, w, c)
    got = bilinear_fwd(ctx, guards, x, None, None, O.ACT_NONE, fy, fx, "dense", {"bilinear_fwd_kernel": 1})
    fwd = ratio(got, MC.up(x, fy, fx), 0.0)
    n, h, w, c, fy, fx = MC.BILINEAR_BWD_TRIP
    assert MC.ew_blocks(n * h * w * c // 4)["trips"] == 2
    g = MC.bilinear_grad(n, h, w, c)
    got = bilinear_bwd(ctx, guards, g, h, w, fy, fx, 0, "dense", {"bilinear_bwd_kernel": 1})
    report("bilinear", "second trips", fwd=fwd, bwd=ratio(got, g, 0.0))
    finish(ctx, guards)


# ----------------------------------------------------------------------------------------------------------- mask head
def mask_fwd(ctx, guards, dl, dy, shape, weights, want=("prob", "loss")):
    n, h, w, fy, fx = shape
    prob = guards.out((n, h * fy * w * fx, 4)) if "prob" in want else None
    loss = guards.out(n) if "loss" in want else None
    labelled = loss is not None
    kernels = launched(ctx, lambda: ctx.call("ssdseg_mask_head_fwd", dl, n, h, w, 4, fy, fx, dy if labelled else None,
                                             c4(weights) if labelled else None, prob, loss))
    assert kernels == (FWD_KERNELS if labelled else {"mask_head_fwd_kernel": 1}), kernels
    out = {k: b.download() for k, b in (("prob", prob), ("loss", loss)) if b is not None}
    assert not any(poisoned(v) for v in out.values())
    return out


def mask_bwd(ctx, guards, monkeypatch, dl, dy, shape, weights, loss_scale, gather=False, dice=None):
    """dice: (coef buffer, squared); -> dlogits (n, h, w, 4) after asserting the dispatch mirror's kernel"""
    n, h, w, fy, fx = shape
    g = guards.out((n, h, w, 4))
    if gather:
        monkeypatch.setenv("SSDSEG_MASK_BWD", "gather")
    if dice is None:
        call = lambda: ctx.call("ssdseg_mask_head_bwd", dl, n, h, w, 4, fy, fx, dy, c4(weights), loss_scale, g)
    else:
        call = lambda: ctx.call("ssdseg_mask_head_bwd_dice", dl, n, h, w, 4, fy, fx, dy, dice[0], dice[1], loss_scale, g)
    kernels = launched(ctx, call)
    if gather:
        monkeypatch.delenv("SSDSEG_MASK_BWD")
    assert kernels == {MC.mask_bwd_dispatch(n, h, w, fy, fx, gather)[0]: 1}, kernels
    got = g.download()
    assert poisoned(got) == 0
    return got


def tiled(shape):
    return shape[3:] in ((4, 4), (8, 8))


def backward_paths(ctx, guards, monkeypatch, dl, dy, shape, weights, loss_scale, ref, bound, dice=None):
    """the default kernel against float64; for x4 and x8 the gather kernel too: x4 bit-identical, x8 within the bound of it"""
    got = mask_bwd(ctx, guards, monkeypatch, dl, dy, shape, weights, loss_scale, dice=dice)
    ratios = {"dlogits": ratio(got, ref, bound)}
    if tiled(shape):
        gat = mask_bwd(ctx, guards, monkeypatch, dl, dy, shape, weights, loss_scale, gather=True, dice=dice)
        ratios["gather"] = ratio(gat, ref, bound)
        if shape[3] == 4:
            assert same_bits(got, gat), "x4 tile kernel != gather kernel"
        else:
            ratios["split-gather"] = ratio(got, gat, bound)
    return ratios, got


@pytest.mark.parametrize("shape", MC.MASK_SHAPES, ids=tag)
def test_mask_head_cross_entropy_edges(ctx, guards, monkeypatch, shape):
    """every family (the capped grids: clip only) with mixed labels: probabilities, their row sums, the loss with and without stored
    probabilities, probabilities alone, and the backward on every kernel the shape can take.  Row sums: sum_k fl(e_k inv) with
    inv = fl(1 / fl(sum e)) is off 1 by the three additions of the sum, the reciprocal and the mean rounding of the products; the 4 U
    asserted leaves out that all five fall the same way (0.82 of it is the most seen, over 530,000 rows)"""
    families = list(MC.FAMILIES) if shape in MC.MASK_SMALL_SHAPES else ["clip"]
    for k, family in enumerate(families):
        case = MC.mask_case(shape, family)
        assert case is not None, f"no seed of {MC.SEEDS} without an undecidable entry"
        weights, scale = MC.mask_settings(shape, k)
        y, p, bp = case["y"], case["p"], case["bp"]
        dl, dy = guards.inp(case["logits"]), guards.inp(y)
        both = mask_fwd(ctx, guards, dl, dy, shape, weights)
        only_p = mask_fwd(ctx, guards, dl, dy, shape, weights, ("prob",))
        only_l = mask_fwd(ctx, guards, dl, dy, shape, weights, ("loss",))
        assert same_bits(both["prob"], only_p["prob"]) and same_bits(both["loss"], only_l["loss"])
        ref, bound = MC.ce_backward(case, weights, scale)
        ratios, _ = backward_paths(ctx, guards, monkeypatch, dl, dy, shape, weights, scale, ref, bound)
        report("mask_head ce", f"{tag(shape)} {family} seed{case['seed']} scale{scale:g}",
               prob=ratio(both["prob"], p, bp), rowsum=ratio(both["prob"].astype(np.float64).sum(-1), 1.0, 4 * U),
               loss=ratio(both["loss"], MC.ce_ref(y, p, weights), MC.ce_bound(y, p, bp, weights)), **ratios)
        finish(ctx, guards)


@pytest.mark.parametrize("squared", (0, 1), ids=("dice", "dice_square"))
@pytest.mark.parametrize("shape", MC.MASK_SHAPES, ids=tag)
def test_mask_head_dice_edges(ctx, guards, monkeypatch, shape, squared):
    """one-hot labels with void rows, class 3 absent from image 0 and (n > 1) an all-void last image: loss, coefficients, backward;
    the capped grids (256 partial blocks of eight sums folded by mask_dice_final_kernel, a ninth trip and more) on the clip family"""
    n, h, w, fy, fx = shape
    ratios = {}
    for k, family in enumerate(("moderate", "clip") if shape in MC.MASK_SMALL_SHAPES else ("clip",)):
        case = MC.mask_case(shape, family, "dice")
        weights, scale = MC.mask_settings(shape, k + squared)
        y, p, bp = case["y"], case["p"], case["bp"]
        dl, dy = guards.inp(case["logits"]), guards.inp(y)
        prob, loss, coef = guards.out(y.shape), guards.out(n), guards.out((n, 8))
        kernels = launched(ctx, lambda: ctx.call("ssdseg_mask_head_fwd_dice", dl, n, h, w, 4, fy, fx, dy, c4(weights), squared, prob, loss, coef))
        assert kernels == DICE_KERNELS and untouched(prob) + untouched(loss) + untouched(coef) == 0
        loss_ref, coef_ref = MC.dice_ref(y, p, weights, squared)
        ref, bound = MC.dice_backward(case, weights, squared, scale)
        back, _ = backward_paths(ctx, guards, monkeypatch, dl, dy, shape, weights, scale, ref, bound, dice=(coef, squared))
        ratios.update({f"{family}-{name}": v for name, v in back.items()})
        ratios[f"{family}-prob"] = ratio(prob.download(), p, bp)
        ratios[f"{family}-loss"] = ratio(loss.download(), loss_ref, MC.dice_bound(y, p, bp, weights, squared))
        ratios[f"{family}-coef"] = ratio(coef.download(), coef_ref, MC.SECOND_ORDER * MC.dice_coef_error(y, p, bp, weights, squared))
        loss_only = guards.out(n)
        ctx.call("ssdseg_mask_head_fwd_dice", dl, n, h, w, 4, fy, fx, dy, c4(weights), squared, None, loss_only, None)
        assert same_bits(loss_only.download(), loss.download())
    report("mask_head dice", f"{tag(shape)} squared{squared}", **ratios)
    finish(ctx, guards)


@pytest.mark.parametrize("cls", (0, 1), ids=("above-hi", "below-lo"))
@pytest.mark.parametrize("shape", MC.PINNED_SHAPES, ids=tag)
def test_mask_head_pinned_clip_cases(ctx, guards, monkeypatch, shape, cls):
    """constant logits (40, 0, 0, 0): every labelled probability is outside the clip interval, every dlogits element exactly 0, the
    loss npix w (-log bound)"""
    case = MC.pinned_case(shape, cls)
    y, p, bp = case["y"], case["p"], case["bp"]
    dl, dy = guards.inp(case["logits"]), guards.inp(y)
    out = mask_fwd(ctx, guards, dl, dy, shape, MC.CW)
    assert (out["prob"][..., 0] == 1.0).all()
    want = y.shape[1] * float(F32(MC.CW[cls])) * -np.log(MC.HI if cls == 0 else MC.LO)
    assert np.allclose(MC.ce_ref(y, p, MC.CW), want, rtol=1e-12, atol=0)
    ratios, got = backward_paths(ctx, guards, monkeypatch, dl, dy, shape, MC.CW, 0.5, np.zeros(case["logits"].shape), 0.0)
    assert not got.any()
    report("mask_head pinned", f"{tag(shape)} class{cls}", loss=ratio(out["loss"], want, MC.ce_bound(y, p, bp, MC.CW)), **ratios)
    finish(ctx, guards)


@pytest.mark.parametrize("shape", [MC.MASK_X4_SHAPES[5], MC.MASK_X8_SHAPES[5], MC.MASK_GATHER_SHAPES[1], MC.MASK_GATHER_SHAPES[2]], ids=tag)
def test_mask_head_exact_zeros(ctx, guards, monkeypatch, shape):
    """all-zero weights; an all-void image; loss_scale 0: the loss is 0 and every gradient element is 0 (values, not the sign of zero)"""
    n, h, w, fy, fx = shape
    zeros = np.zeros((n, h, w, 4))
    for family in ("clip", "extreme"):
        case = MC.mask_case(shape, family)
        dl, dy = guards.inp(case["logits"]), guards.inp(case["y"])
        assert not mask_fwd(ctx, guards, dl, dy, shape, MC.CW_NONE)["loss"].any()
        for scale, weights in ((0.5, MC.CW_NONE), (0.0, MC.CW)):
            _, got = backward_paths(ctx, guards, monkeypatch, dl, dy, shape, weights, scale, zeros, 0.0)
            assert not got.any()
        for squared in (0, 1):
            loss, coef = guards.out(n), guards.out((n, 8))
            ctx.call("ssdseg_mask_head_fwd_dice", dl, n, h, w, 4, fy, fx, dy, c4(MC.CW_NONE), squared, None, loss, coef)
            assert not loss.download().any() and not coef.download().any()
            _, got = backward_paths(ctx, guards, monkeypatch, dl, dy, shape, None, 0.5, zeros, 0.0, dice=(coef, squared))
            assert not got.any()
            ctx.call("ssdseg_mask_head_fwd_dice", dl, n, h, w, 4, fy, fx, dy, c4(MC.CW), squared, None, loss, coef)
            _, got = backward_paths(ctx, guards, monkeypatch, dl, dy, shape, None, 0.0, zeros, 0.0, dice=(coef, squared))
            assert not got.any()
        if n > 1:       # the dice labels end with an all-void image: under cross-entropy its loss and its gradient are 0
            void = MC.mask_case(shape, family, "dice")
            assert not void["y"][-1].any()
            dv = guards.inp(void["y"])
            dlv = guards.inp(void["logits"])
            out = mask_fwd(ctx, guards, dlv, dv, shape, MC.CW)
            assert out["loss"][-1] == 0.0 and out["loss"][0] != 0.0
            got = mask_bwd(ctx, guards, monkeypatch, dlv, dv, shape, MC.CW, -1.0)
            assert not got[-1].any() and got[0].any()
        finish(ctx, guards)


@pytest.mark.parametrize("shape", [(3, 15, 33, 4, 4), (3, 7, 17, 8, 8), (3, 4, 3, 3, 5)], ids=tag)
def test_mask_head_batch_independence(ctx, guards, monkeypatch, shape):
    """an image's prob, loss and dlogits are bit-identical at batch positions 0 and n - 1, cross-entropy and both dice modes"""
    n, h, w, fy, fx = shape
    one = (1,) + shape[1:]
    images = [MC.mask_case(one, family) for family in ("clip", "moderate", "extreme")]
    results = []
    for order in ((0, 1, 2), (2, 1, 0)):
        logits = np.concatenate([images[i]["logits"] for i in order])
        y = np.concatenate([images[i]["y"] for i in order])
        dl, dy = guards.inp(logits), guards.inp(y)
        out = mask_fwd(ctx, guards, dl, dy, shape, MC.CW)
        got = [out["prob"], out["loss"], mask_bwd(ctx, guards, monkeypatch, dl, dy, shape, MC.CW, 0.5)]
        for squared in (0, 1):
            loss, coef = guards.out(n), guards.out((n, 8))
            ctx.call("ssdseg_mask_head_fwd_dice", dl, n, h, w, 4, fy, fx, dy, c4(MC.CW), squared, None, loss, coef)
            got += [loss.download(), coef.download(), mask_bwd(ctx, guards, monkeypatch, dl, dy, shape, None, 0.5, dice=(coef, squared))]
        results.append(got)
    for a, b in zip(*results):
        assert same_bits(a[0], b[2]) and same_bits(a[2], b[0]) and same_bits(a[1], b[1])
    finish(ctx, guards)


BOOTSTRAP_SHAPES = MC.MASK_GATHER_SHAPES + [MC.MASK_X4_SHAPES[0]]


@pytest.mark.parametrize("shape", BOOTSTRAP_SHAPES, ids=tag)
def test_mask_head_bootstrap_gather_shapes(ctx, guards, monkeypatch, shape):
    """fy != fx, non-power-of-two factors and a 1 x 1 source at x4.  keep = npix: the stored pixel losses are the cross-entropy's
    terms, prob and dlogits equal the cross-entropy's bit for bit, and the loss is another summation of the same terms (within the
    cross-entropy's bound of the reference, not its bits).  keep = 1 on the clip family: the loss is the largest per-pixel term,
    times the number of pixels tied at it"""
    n, h, w, fy, fx = shape
    case = MC.mask_case(shape, "clip")
    y, p, bp = case["y"], case["p"], case["bp"]
    npix = y.shape[1]
    dl, dy = guards.inp(case["logits"]), guards.inp(y)

    def forward(keep):
        outs = dict(prob=guards.out(y.shape), pixel_loss=guards.out((n, npix)), thresh=guards.out(n), kept=guards.out(n, np.int32), loss=guards.out(n))
        ctx.call("ssdseg_mask_head_fwd_bootstrap", dl, n, h, w, 4, fy, fx, dy, c4(MC.CW), keep,
                 outs["prob"], outs["pixel_loss"], outs["thresh"], outs["kept"], outs["loss"])
        assert not any(untouched(b) for b in outs.values())
        return outs, {k: b.download() for k, b in outs.items()}
    outs, got = forward(npix)
    ce = mask_fwd(ctx, guards, dl, dy, shape, MC.CW)
    assert same_bits(got["prob"], ce["prob"]) and (got["kept"] == npix).all()
    # a pixel's four terms: the bound of the cross-entropy with one pixel per image (a chain of one)
    term_bound = MC.ce_bound(y.reshape(-1, 1, 4), p.reshape(-1, 1, 4), bp.reshape(-1, 1, 4), MC.CW).reshape(n, npix)
    pixel_ref = MC.ce_pixel_ref(y, p, MC.CW)
    ratios = dict(pixel=ratio(got["pixel_loss"], pixel_ref, term_bound), loss=ratio(got["loss"], MC.ce_ref(y, p, MC.CW), MC.ce_bound(y, p, bp, MC.CW)))
    g = guards.out((n, h, w, 4))
    kernels = launched(ctx, lambda: ctx.call("ssdseg_mask_head_bwd_bootstrap", dl, n, h, w, 4, fy, fx, dy, c4(MC.CW), outs["pixel_loss"],
                                             outs["thresh"], 0.5, g))
    assert kernels == {MC.mask_bwd_dispatch(*shape)[0]: 1}
    assert same_bits(g.download(), mask_bwd(ctx, guards, monkeypatch, dl, dy, shape, MC.CW, 0.5))
    _, top = forward(1)
    largest = top["pixel_loss"].max(axis=1)
    tied = (top["pixel_loss"] == largest[:, None]).sum(axis=1)
    assert same_bits(top["thresh"], largest) and np.array_equal(top["kept"], tied)
    # one kept pixel: the sum is that term and zeros, exact; pixels tied at it: a float32 chain of at most a thread's trips and 8 levels
    chain = MC.gamma(-(-npix // 256) + 8) * (tied > 1)
    ratios["keep1"] = ratio(top["loss"], tied * largest.astype(np.float64), chain * tied * largest)
    ratios["largest"] = ratio(largest, pixel_ref.max(axis=1), term_bound.max(axis=1))
    report("mask_head bootstrap", tag(shape), **ratios)
    finish(ctx, guards)


# ---------------------------------------------------------------------------------------------------- argument contracts
def refused(ctx, name, *args):
    """rejected() for the two bilinear forwards, whose checks report under the name of the function they share"""
    from ssdseglib import _hip as H
    with pytest.raises(H.SsdsegError, match=f"{name} failed with code .*bilinear_fwd_impl: invalid argument"):
        ctx.call(name, *args)


def test_argument_contracts(ctx, guards):
    """every call is rejected with the library's argument error before anything is launched: the outputs stay poison"""
    from ssdseglib import _hip as H
    n, h, w, f = 1, 2, 2, 2
    x = guards.inp(np.zeros((n, h, w, 4), F32))
    y = guards.inp(np.zeros((n, h * f * w * f, 4), F32))
    prob, loss, coef, g = guards.out((n, h * f * w * f, 4)), guards.out(n), guards.out((n, 8)), guards.out((n, h, w, 4))
    pl, thr, kept = guards.out((n, h * f * w * f)), guards.out(n), guards.out(n, np.int32)
    wide = guards.out((n * h * f * w * f, 8))
    cw = c4(MC.CW)
    entries = {
        "ssdseg_mask_head_fwd": lambda a: (a["logits"], a["n"], h, w, a["c"], a["fy"], a["fx"], a["y"], cw, prob, loss),
        "ssdseg_mask_head_bwd": lambda a: (a["logits"], a["n"], h, w, a["c"], a["fy"], a["fx"], a["y"], cw, 0.5, a["out"]),
        "ssdseg_mask_head_fwd_dice": lambda a: (a["logits"], a["n"], h, w, a["c"], a["fy"], a["fx"], a["y"], cw, 0, prob, loss, coef),
        "ssdseg_mask_head_bwd_dice": lambda a: (a["logits"], a["n"], h, w, a["c"], a["fy"], a["fx"], a["y"], coef, 0, 0.5, a["out"]),
        "ssdseg_mask_head_fwd_bootstrap": lambda a: (a["logits"], a["n"], h, w, a["c"], a["fy"], a["fx"], a["y"], cw, 1, prob, pl, thr, kept, loss),
        "ssdseg_mask_head_bwd_bootstrap": lambda a: (a["logits"], a["n"], h, w, a["c"], a["fy"], a["fx"], a["y"], cw, pl, thr, 0.5, a["out"]),
    }
    good = dict(logits=x, n=n, c=4, fy=f, fx=f, y=y, out=g)

    def calls():
        for name, args in entries.items():
            for change in (dict(c=8), dict(fy=0), dict(fx=0), dict(fx=-1), dict(logits=None), dict(y=None), dict(n=0)):
                rejected(ctx, name, *args({**good, **change}))
            if "bwd" in name:
                rejected(ctx, name, *args({**good, "out": None}))
            else:
                rejected(ctx, name, *args({**good, "n": 65536}))                                   # n is gridDim.y
        rejected(ctx, "ssdseg_mask_head_fwd", x, n, h, w, 4, f, f, y, None, prob, loss)            # a loss without weights
        rejected(ctx, "ssdseg_mask_head_fwd_dice", x, n, h, w, 4, f, f, y, None, 0, prob, loss, coef)
        rejected(ctx, "ssdseg_mask_head_fwd_dice", x, n, h, w, 4, f, f, y, cw, 0, prob, None, None)
        rejected(ctx, "ssdseg_mask_head_bwd_dice", x, n, h, w, 4, f, f, y, None, 0, 0.5, g)
        rejected(ctx, "ssdseg_mask_head_fwd_bootstrap", x, n, h, w, 4, f, f, y, cw, 0, prob, pl, thr, kept, loss)       # keep < 1
        rejected(ctx, "ssdseg_mask_head_fwd_bootstrap", x, n, h, w, 4, f, f, y, cw, 17, prob, pl, thr, kept, loss)      # keep > npix
        rejected(ctx, "ssdseg_mask_head_fwd_bootstrap", x, n, h, w, 4, f, f, y, cw, 1, prob, None, thr, kept, loss)
        rejected(ctx, "ssdseg_mask_head_fwd_bootstrap", x, n, h, w, 4, f, f, y, cw, 1, prob, pl, None, kept, loss)
        rejected(ctx, "ssdseg_mask_head_bwd_bootstrap", x, n, h, w, 4, f, f, y, cw, None, thr, 0.5, g)
        rejected(ctx, "ssdseg_mask_head_bwd_bootstrap", x, n, h, w, 4, f, f, y, cw, pl, None, 0.5, g)
        for name in ("ssdseg_bilinear_fwd", "ssdseg_bilinear_fwd_padded"):
            refused(ctx, name, H.view(x), 0, wide, 8, n, h, w, 4, f, f)                           # ldx < c
            refused(ctx, name, H.view(x), 6, wide, 8, n, h, w, 4, f, f)                           # ldx % 4 != 0
            refused(ctx, name, H.view(x), 4, wide, 0, n, h, w, 4, f, f)                           # ldo < c
            refused(ctx, name, H.view(x), 4, wide, 6, n, h, w, 4, f, f)                           # ldo % 4 != 0
            refused(ctx, name, H.view(x), 4, None, 8, n, h, w, 4, f, f)
            refused(ctx, name, H.view(None), 4, wide, 8, n, h, w, 4, f, f)
            refused(ctx, name, H.view(x, y, None), 4, wide, 8, n, h, w, 4, f, f)                  # a view with only a scale
            refused(ctx, name, H.view(x), 4, wide, 8, n, h, w, 6, f, f)                           # c % 4 != 0
            refused(ctx, name, H.view(x), 4, wide, 8, n, h, w, 4, 0, f)
            refused(ctx, name, H.view(x), 4, wide, 8, n, 0, w, 4, f, f)
        rejected(ctx, "ssdseg_bilinear_bwd", y, 0, g, 4, n, h, w, 4, f, f, 0)                      # ldg < c
        rejected(ctx, "ssdseg_bilinear_bwd", y, 6, g, 4, n, h, w, 4, f, f, 0)
        rejected(ctx, "ssdseg_bilinear_bwd", y, 4, g, 0, n, h, w, 4, f, f, 0)                      # ldx < c
        rejected(ctx, "ssdseg_bilinear_bwd", y, 4, g, 6, n, h, w, 4, f, f, 0)
        rejected(ctx, "ssdseg_bilinear_bwd", None, 4, g, 4, n, h, w, 4, f, f, 0)
        rejected(ctx, "ssdseg_bilinear_bwd", y, 4, None, 4, n, h, w, 4, f, f, 0)
        rejected(ctx, "ssdseg_bilinear_bwd", y, 4, g, 4, n, h, w, 4, f, 0, 0)
        rejected(ctx, "ssdseg_bilinear_bwd", y, 4, g, 4, 0, h, w, 4, f, f, 0)
    assert launched(ctx, calls) == {}
    for buf in (prob, loss, coef, g, pl, thr, kept, wide):
        assert untouched(buf) == buf.size
    finish(ctx, guards)
