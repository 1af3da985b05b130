"""GPU parity of the kernels that run after the convs and around the model, at their edges (through the C-ABI) vs float64.

ssdseg_dice_loss (csrc/losses.hip), ssdseg_metric_mask_iou (csrc/mask_head.hip), ssdseg_metric_label_accuracy, ssdseg_metric_box_iou,
ssdseg_head_gather, ssdseg_softmax_rows (csrc/heads.hip), ssdseg_gap_fwd / _bwd and ssdseg_bilinear_bwd from a 1 x 1 source
(csrc/resize.hip), ssdseg_channel_shuffle, ssdseg_channel_gather, ssdseg_copy2d, ssdseg_copy2d_batch (csrc/shuffle.hip) on the cases of
tests/_tail_cases.py: more than one partial block and the 64-block caps, more than 64 images, every chunk count of the pixel sum and
both of its launch forms, arg-max ties, denormal and negative-zero targets, padded gather entries, row pitches with a gap, a second
grid-stride trip, and the argument contracts.  tests/test_cpu_tail_cases.py vets the references, the cases and the bounds.  Every
buffer is guarded (tests/_guard.py).

The bounds are derived, not tuned; the derivations stand with the functions in tests/_tail_cases.py.  U = 2^-24, ULP = 2^-23.

  moves         head_gather (and its reverse), channel_shuffle, channel_gather, copy2d, copy2d_batch without a view: exact.
  moves + view  act(fma(s, x, t)) is one rounding of the float64 pre-activation, the clamp never moves it further from the float64
                clamp: 1 ULP of |s x| + |t|; accumulate adds one rounding of the sum (U |result|); a padded gather entry is exact.
  softmax_rows  per probability, relative: U (2 |z_c - max| + 2): the rounding of expf's argument a, the error U |a| of expf as this
                library is built (under -ffp-contract=fast the rounding of a log2(e) is left uncompensated, see softmax_bound;
                ocml's 1 ulp holds without the flag), the exp2 (1 ulp); the same p-weighted for the sum, 3 roundings of the sum, the reciprocal, the product (softmax_bound); + 2^-126 where expf
                underflows.
  two-level sums  gamma(L) of the sum of absolute terms, L = trips of a thread + 8 tree levels (or the blockDim.y fold of
                gap_fwd_kernel) + nblk / chunks of the finish + the roundings that form a term, all from the launch mirrors; then
                through the closed form: dice through r = (2 I + e) / (T + e) (dice_bound), the Jaccard through I / D with
                D = T - I + e >= T / 2 (iou_bound), from logits with the per-pixel error of softmax(bilinear(logits))
                (logits_prob_error), the box IoU with the per-anchor error of the decoded corners (box_bound), the accuracy with
                exact integer counts and 5 roundings of the weighted sum (accuracy_bound).

Run with -s for the largest error / bound ratio of every case (DESIGN.md records them).
"""
import numpy as np
import pytest

import _tail_cases as TC
from oracle import np_ops as O
from _guard import BODY_WORD, INPUT_WORD, guards  # noqa: F401  (fixture)
from _edge_helpers import c4, dev_view, finish, launched, ratio, rejected, reporter, same_bits, untouched

pytestmark = pytest.mark.gpu

F32 = np.float32
U, ULP = TC.U, TC.ULP


report = reporter("tail-edges")


# ------------------------------------------------------------------------------------------------------------------ dice
def run_dice(ctx, guards, y, p, weights, mode):
    n, hw = y.shape[:2]
    loss = guards.out(n)
    yb, pb = guards.inp(y), guards.inp(p)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_dice_loss", yb, pb, n, hw, 4, c4(weights), mode, loss))
    assert kernels == {"dice_partial_kernel": 1, "dice_finish_kernel": 1}
    return loss.download()


@pytest.mark.parametrize("mode", TC.DICE_MODES)
@pytest.mark.parametrize("n,hw", TC.DICE_SHAPES)
def test_dice_loss_edges(ctx, guards, n, hw, mode):
    y, p = TC.dice_case(n, hw)
    ratios = {}
    for name, w in (("cw", TC.CW), ("zero-weight", TC.CW_ZERO)):
        ratios[name] = ratio(run_dice(ctx, guards, y, p, w, mode), TC.dice_ref(y, p, w, mode), TC.dice_bound(y, p, w, mode))
    report("dice_loss", f"n{n} hw{hw} mode{mode}", **ratios)
    finish(ctx, guards)


@pytest.mark.parametrize("mode", (0, 1))
def test_dice_loss_absent_class(ctx, guards, mode):
    """class 3 absent from y with p exactly 0: (0 + e) / (0 + e) = 1 and the term is exactly 0"""
    y, p = TC.dice_case(3, 4100, "absent")
    only = run_dice(ctx, guards, y, p, (0.0, 0.0, 0.0, 1.0), mode)
    assert only[0] == 0.0 and only[1] != 0.0
    report("dice_loss", f"absent-class mode{mode}", cw=ratio(run_dice(ctx, guards, y, p, TC.CW, mode), TC.dice_ref(y, p, TC.CW, mode),
                                                             TC.dice_bound(y, p, TC.CW, mode)))
    finish(ctx, guards)


def test_dice_loss_mode2_clip_edges(ctx, guards):
    y, p = TC.dice_case(2, 40, "clip")
    report("dice_loss", "clip-edges mode2", cw=ratio(run_dice(ctx, guards, y, p, TC.CW, 2), TC.dice_ref(y, p, TC.CW, 2), TC.dice_bound(y, p, TC.CW, 2)))
    finish(ctx, guards)


# -------------------------------------------------------------------------------------------------------------- mask IoU
def run_mask_iou(ctx, guards, src, n, h, w, fy, fx, from_logits, y, weights):
    out = guards.out(n)
    sb, yb = guards.inp(src), guards.inp(y)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_metric_mask_iou", sb, n, h, w, 4, fy, fx, from_logits, yb, c4(weights), out))
    assert kernels.get("mask_iou_finish_kernel") == 1 and sorted(kernels.values()) == [1, 1], kernels
    return out.download()


@pytest.mark.parametrize("n,h,w", TC.IOU_PROB_SHAPES)
def test_mask_iou_from_probabilities_edges(ctx, guards, n, h, w):
    y, p = TC.iou_prob_case(n, h, w)
    ratios = {}
    for name, wt in (("cw", TC.CW), ("zero-weight", TC.CW_ZERO)):
        ratios[name] = ratio(run_mask_iou(ctx, guards, p, n, h, w, 1, 1, 0, y, wt), TC.iou_ref(y, p, wt), TC.iou_bound(y, p, wt))
    if h * w >= 8:      # class 2 is absent from y in image 0: its term is exactly 0
        assert run_mask_iou(ctx, guards, p, n, h, w, 1, 1, 0, y, (0.0, 0.0, 1.0, 0.0))[0] == 0.0
    report("mask_iou", f"prob n{n} {h}x{w}", **ratios)
    finish(ctx, guards)


@pytest.mark.parametrize("n,h,w,fy,fx", TC.IOU_LOGIT_SHAPES)
def test_mask_iou_from_logits_edges(ctx, guards, n, h, w, fy, fx):
    y, logits, p = TC.iou_logit_case(n, h, w, fy, fx)
    perr = TC.logits_prob_error(TC.LOGIT_MAG)
    ratios = {}
    for name, wt in (("cw", TC.CW), ("zero-weight", TC.CW_ZERO)):
        ratios[name] = ratio(run_mask_iou(ctx, guards, logits, n, h, w, fy, fx, 1, y, wt), TC.iou_ref(y, p, wt), TC.iou_bound(y, p, wt, perr))
    report("mask_iou", f"logits n{n} {h}x{w} x{fy}x{fx}", **ratios)
    finish(ctx, guards)


# ------------------------------------------------------------------------------------------------------- label accuracy
@pytest.mark.parametrize("b,a", TC.ACC_SHAPES)
def test_label_accuracy_edges(ctx, guards, b, a):
    t, p, _ = TC.accuracy_case(b, a)
    tb, pb = guards.inp(t), guards.inp(p)
    ratios = {}
    for name, w in (("lw", TC.LW), ("cw", TC.CW)):
        out = guards.out(b)
        kernels = launched(ctx, lambda: ctx.call("ssdseg_metric_label_accuracy", tb, pb, b, a, 4, c4(w), out))
        assert kernels == {"label_accuracy_kernel": 1}
        ratios[name] = ratio(out.download(), TC.accuracy_ref(t, p, w), TC.accuracy_bound(t, p, w))
    report("label_accuracy", f"b{b} a{a}", **ratios)
    finish(ctx, guards)


# -------------------------------------------------------------------------------------------------------------- box IoU
@pytest.mark.parametrize("a", TC.BOX_SIZES)
def test_box_iou_edges(ctx, guards, a):
    t, p, anchors, _ = TC.box_case(a)
    b = t.shape[0]
    out = guards.out(b)
    tb, pb, ab = guards.inp(t), guards.inp(p), guards.inp(np.stack(anchors, axis=-1))
    kernels = launched(ctx, lambda: ctx.call("ssdseg_metric_box_iou", tb, pb, ab, c4(TC.STDS), b, a, out))
    assert kernels == {"box_iou_kernel": 1}
    got, ref, bound = out.download(), TC.box_ref(t, p, anchors), TC.box_bound(t, p, anchors)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).tolist() == [True, False, False, False]
    ok = ~np.isnan(ref)
    report("box_iou", f"a{a}", **{name: ratio(got[i], ref[i], bound[i]) for i, name in enumerate(TC.BOX_IMAGES) if ok[i]})
    finish(ctx, guards)


# ---------------------------------------------------------------------------------------------------------- head gather
@pytest.mark.parametrize("act", (None,) + TC.ACTS, ids=lambda a: "plain" if a is None else TC.ACT_NAMES[a])
@pytest.mark.parametrize("b,cells,c,off,total", TC.GATHER_SHAPES[:4])
def test_head_gather_edges(ctx, guards, b, cells, c, off, total, act):
    x = TC.seeded(30, b, cells, c).normal(0, 2, (b, cells, c)).astype(F32)
    s, t = (None, None) if act is None else TC.view_params(c, 5)
    ref, written, mag = TC.head_gather_ref(x, s, t, O.ACT_NONE if act is None else act, off, total)
    out = guards.out((b, total, 4))
    view = dev_view(guards, x, s, t, O.ACT_NONE if act is None else act)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_head_gather", view, out, b, cells * c, c, off * 4, total * 4, 0))
    assert kernels == {"head_gather_kernel": 1}
    got = out.download()
    assert (got.view(np.uint32)[~written] == np.uint32(BODY_WORD)).all(), "an element outside [off, off + n) was written"
    report("head_gather", f"b{b} cells{cells} c{c} off{off} total{total} {'plain' if act is None else TC.ACT_NAMES[act]}",
           out=ratio(got[written], ref[written], ULP * mag[written]))
    finish(ctx, guards)


@pytest.mark.parametrize("b,cells,c,off,total", TC.GATHER_SHAPES)
def test_head_gather_round_trip(ctx, guards, b, cells, c, off, total):
    from ssdseglib import _hip as H
    x = TC.seeded(31, b, c, off).standard_normal((b, cells, c), dtype=F32)
    x[0, 0, 1], x[-1, -1, -1] = -0.0, 2.0 ** -140          # a move keeps the sign of a zero and a denormal
    out = guards.out((b, total, 4))
    ctx.call("ssdseg_head_gather", dev_view(guards, x), out, b, cells * c, c, off * 4, total * 4, 0)
    n = cells * c // 4
    assert same_bits(out.download()[:, off:off + n], x.reshape(b, n, 4))
    assert untouched(out) == b * (total - n) * 4
    back = guards.out((b, cells, c))
    ctx.call("ssdseg_head_gather", H.view(out), back, b, cells * c, c, off * 4, total * 4, 1)
    assert same_bits(back.download(), x)
    finish(ctx, guards)


# -------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("rows,spread", [(r, s) for r in TC.SOFTMAX_ROWS[:4] for s in TC.SOFTMAX_SPREADS] + [(TC.SOFTMAX_ROWS[4], 30.0)])
def test_softmax_rows_edges(ctx, guards, rows, spread):
    z = TC.softmax_case(rows, spread)
    out = guards.out((rows, 4))
    view = dev_view(guards, z)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_softmax_rows", view, out, rows, 4))
    assert kernels == {"softmax_rows4_kernel": 1}
    got, ref, bound = out.download(), TC.softmax_ref(z), TC.softmax_bound(z)
    assert (got[0] == 0.25).all()
    if spread == 200.0 and rows > 1:
        assert got[1, 0] == 1.0 and ref[1, 0] == 1.0
    report("softmax_rows", f"rows{rows} spread{spread:g}", p=ratio(got, ref, bound),
           rowsum=ratio(got.astype(np.float64).sum(-1), np.ones(rows), bound.sum(-1)))
    finish(ctx, guards)


def test_softmax_rows_common_offset(ctx, guards):
    z = TC.softmax_case(257, 1.0, offset=1e30)
    out = guards.out((257, 4))
    ctx.call("ssdseg_softmax_rows", dev_view(guards, z), out, 257, 4)
    report("softmax_rows", "offset 1e30", p=ratio(out.download(), TC.softmax_ref(z), TC.softmax_bound(z)))
    finish(ctx, guards)


def test_softmax_rows_affine_relu6_view(ctx, guards):
    """the SSD confidence head: softmax of relu6(s x + t); a logit carries the view's rounding, U (|s x| + |t|)"""
    rows = 257
    x = TC.seeded(32).normal(0, 3, (rows, 4)).astype(F32)
    s, t = TC.view_params(4, 6)
    zin, mag = TC.view_ref(x, s, t, O.ACT_RELU6)
    out = guards.out((rows, 4))
    ctx.call("ssdseg_softmax_rows", dev_view(guards, x, s, t, O.ACT_RELU6), out, rows, 4)
    assert (zin == 0).any() and (zin == 6).any()
    report("softmax_rows", "affine+relu6", p=ratio(out.download(), TC.softmax_ref(zin), TC.softmax_bound(zin, zerr=U * mag.max(-1, keepdims=True))))
    finish(ctx, guards)


# ------------------------------------------------------------------------------------------------- average pool, pixel sum
@pytest.mark.parametrize("affine", (False, True), ids=("plain", "affine+relu6"))
@pytest.mark.parametrize("n,hw,c", TC.GAP_SHAPES)
def test_gap_fwd_edges(ctx, guards, n, hw, c, affine):
    x = TC.gap_case(n, hw, c)
    s, t, act = (*TC.view_params(c, 2), O.ACT_RELU6) if affine else (None, None, O.ACT_NONE)
    la = TC.pixel_sum_launch(n, hw, c)
    out = guards.out((n, c))
    view = dev_view(guards, x, s, t, act)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_gap_fwd", view, out, n, hw, c))
    assert kernels == la["kernels"], (kernels, la)
    a, _ = TC.view_ref(x, s, t, act)
    # the view's rounding, the multiplier 1 / hw as a float32 and its product: 3 more roundings
    report("gap_fwd", f"n{n} hw{hw} c{c} chunks{la['chunks']} {'affine' if affine else 'plain'}",
           out=ratio(out.download(), O.gap_fwd(a[:, :, None])[:, 0, 0], TC.pixel_sum_bound(a, la, 3) / hw))
    finish(ctx, guards)


@pytest.mark.parametrize("form", ("dense", "pitched", "slice"))
@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("n,c,fy,fx", TC.BILINEAR_1X1_SHAPES)
def test_bilinear_bwd_from_1x1_edges(ctx, guards, n, c, fy, fx, accumulate, form):
    """dense: ldg = ldx = c; pitched: both > c with gap columns; slice: both operands are channel slices at column 4 of wider
    (concat) buffers, the pitch comes with a base-pointer offset"""
    hw = fy * fx
    rng = TC.seeded(33, n, c, fy, fx)
    g = rng.normal(0, 1, (n, hw, c)).astype(F32)
    base = rng.normal(0, 1, (n, c)).astype(F32)
    ldg, ldx = {"dense": (c, c), "pitched": (c + 4, c + 8), "slice": (c + 8, c + 8)}[form]
    la = TC.pixel_sum_launch(n, hw, c, accumulate, form != "dense")
    if form == "slice":
        gw = np.full((n * hw, ldg), INPUT_WORD, np.uint32).view(F32)
        gw[:, 4:4 + c] = g.reshape(n * hw, c)
        gwide, dwide = guards.inp(gw), guards.out((n, ldx))
        if accumulate:
            dw = np.full((n, ldx), BODY_WORD, np.uint32).view(F32)
            dw[:, 4:4 + c] = base
            dwide.upload(dw)
        gb, dx = gwide.view(4, (gwide.size - 4,)), dwide.view(4, (dwide.size - 4,))
    else:
        gb = guards.inp(g.reshape(n * hw, c), ld=ldg)
        dx = guards.out((n, c), ld=ldx)
        if accumulate:
            dx.upload(base)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_bilinear_bwd", gb, ldg, dx, ldx, n, 1, 1, c, fy, fx, accumulate))
    assert kernels == la["kernels"], (kernels, la)
    if form == "slice":
        wide = dwide.download()
        got = wide[:, 4:4 + c]
        assert (wide[:, :4].view(np.uint32) == BODY_WORD).all() and (wide[:, 4 + c:].view(np.uint32) == BODY_WORD).all()
    else:
        got = dx.download()
    g64 = g.astype(np.float64)
    ref = O.bilinear_bwd(g64.reshape(n, fy, fx, c), fy, fx).reshape(n, c) + (base if accumulate else 0.0)
    bound = TC.pixel_sum_bound(g64, la, 0) + (U * np.abs(ref) if accumulate else 0.0)
    report("bilinear_bwd 1x1", f"n{n} c{c} x{fy}x{fx} acc{accumulate} {form} chunks{la['chunks']}", dx=ratio(got, ref, bound))
    finish(ctx, guards)


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("n,hw,c", TC.GAP_BWD_SHAPES)
def test_gap_bwd_edges(ctx, guards, n, hw, c, accumulate):
    rng = TC.seeded(34, n, hw, c)
    g = rng.normal(0, 1, (n, 1, 1, c)).astype(F32)
    dx = guards.out((n, hw, c))
    base = None
    if accumulate:
        base = rng.standard_normal((n, hw, c), dtype=F32)
        dx.upload(base)
    else:       # overwrite mode must not read the destination: it stays poison until the call
        assert untouched(dx) == n * hw * c
    gb = guards.inp(g)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_gap_bwd", gb, dx, n, hw, c, accumulate))
    assert kernels == {"gap_bwd_kernel": 1}
    spread = O.gap_bwd(g.astype(np.float64), 1, hw).reshape(n, hw, c)
    ref = spread + (base if accumulate else 0.0)
    # 1 / hw as a float32 and the product: 2 U; the sum with the previous contents one more
    bound = 2 * U * np.abs(spread) + (U * np.abs(ref) if accumulate else 0.0)
    report("gap_bwd", f"n{n} hw{hw} c{c} acc{accumulate}", dx=ratio(dx.download(), ref, bound))
    finish(ctx, guards)


# ------------------------------------------------------------------------------------------------------ channel shuffle
# every shape dense, with either pitch and with both; the second grid-stride trip dense and with both
SHUFFLE_RUNS = [shape + gaps for shape in TC.SHUFFLE_SHAPES for gaps in ((0, 0), (3, 0), (0, 5), (3, 5))
                if shape[0] <= 1000 or gaps in ((0, 0), (3, 5))]


@pytest.mark.parametrize("m,c,groups,gi,go", SHUFFLE_RUNS)
def test_channel_shuffle_edges(ctx, guards, m, c, groups, gi, go):
    from ssdseglib import _hip as H
    x = TC.seeded(35, m, c).standard_normal((m, c), dtype=F32)
    x[0, 1], x[-1, -1] = -0.0, 2.0 ** -140                 # a move keeps the sign of a zero and a denormal
    ldi, ldo = c + gi, c + go
    xb = guards.inp(x, ld=ldi)
    fwd = guards.out((m, c), ld=ldo)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_channel_shuffle", H.view(xb), ldi, fwd, ldo, m, c, groups, 0))
    assert kernels == {"shuffle_kernel": 1}
    assert same_bits(fwd.download(), TC.shuffle_ref(x, groups))
    inv = guards.out((m, c), ld=ldo)
    ctx.call("ssdseg_channel_shuffle", H.view(xb), ldi, inv, ldo, m, c, groups, 1)
    assert same_bits(inv.download(), TC.shuffle_ref(x, groups, inverse=True))
    back = guards.out((m, c), ld=ldi)
    ctx.call("ssdseg_channel_shuffle", H.view(fwd), ldo, back, ldi, m, c, groups, 1)
    assert same_bits(back.download(), x)
    s, t = TC.view_params(c, 7)
    sb, tb = guards.inp(s), guards.inp(t)
    ratios = {}
    for act in (TC.ACTS if m <= 1000 else (O.ACT_RELU6,)):
        out = guards.out((m, c), ld=ldo)
        ctx.call("ssdseg_channel_shuffle", H.view(xb, sb, tb, act), ldi, out, ldo, m, c, groups, 0)
        val, mag = TC.view_ref(x, s, t, act)        # scale and shift belong to the source channel
        idx = TC.shuffle_index(c, groups)
        ratios[TC.ACT_NAMES[act]] = ratio(out.download(), val[:, idx], ULP * mag[:, idx])
    report("channel_shuffle", f"m{m} c{c} g{groups} ldi{ldi} ldo{ldo}", **ratios)
    finish(ctx, guards)


# ------------------------------------------------------------------------------------------------------- channel gather
def run_gather(ctx, guards, m, ldi, table, ldo, accumulate, s, t, act, seed):
    rng = TC.seeded(36, m, ldi, seed)
    x = rng.standard_normal((m, ldi), dtype=F32)
    x[0, 1], x[-1, -1] = -0.0, 2.0 ** -140
    c_out = table.size
    base = rng.standard_normal((m, c_out), dtype=F32) if accumulate else None
    out = guards.out((m, c_out), ld=ldo)
    if accumulate:
        out.upload(base)
    view = dev_view(guards, x, s, t, act)
    tb = guards.inp(table)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_channel_gather", view, ldi, out, ldo, m, c_out, tb, accumulate))
    assert kernels == {"channel_gather_kernel": 1}
    ref, mag = TC.channel_gather_ref(x, table, s, t, act, base)
    got = out.download()
    pad = table < 0
    if pad.any():       # exactly 0, or the previous contents: never act(shift)
        assert same_bits(got[:, pad], base[:, pad] if accumulate else np.zeros((m, int(pad.sum())), F32))
    bound = ULP * mag + (U * np.abs(ref) * ~pad[None] if accumulate else 0.0)       # the sum with the previous contents: one rounding
    return ratio(got, ref, bound)


@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("name", list(TC.gather_tables()))
@pytest.mark.parametrize("m", (1, 300))
def test_channel_gather_edges(ctx, guards, m, name, accumulate):
    ldi, table = TC.gather_tables()[name]
    ldo = table.size + (2 if m == 300 else 0)
    s, t = TC.gather_view_params(ldi, 8)
    ratios = {"plain": run_gather(ctx, guards, m, ldi, table, ldo, accumulate, None, None, O.ACT_NONE, 0)}
    if not accumulate:
        assert ratios["plain"] == 0.0       # a move: exact (under accumulate one rounding of the sum, which float32 NumPy shares)
    for act in TC.ACTS:
        ratios[TC.ACT_NAMES[act]] = run_gather(ctx, guards, m, ldi, table, ldo, accumulate, s, t, act, 1 + act)
    report("channel_gather", f"m{m} {name} acc{accumulate}", **ratios)
    finish(ctx, guards)


def test_channel_gather_second_trip(ctx, guards):
    ldi, table = TC.gather_tables()["reversal"]
    m = 18079
    assert m * table.size > TC.SECOND_TRIP
    s, t = TC.gather_view_params(ldi, 8)
    report("channel_gather", f"m{m} reversal", plain=run_gather(ctx, guards, m, ldi, table, table.size, 0, None, None, O.ACT_NONE, 0),
           relu6=run_gather(ctx, guards, m, ldi, table, table.size, 0, s, t, O.ACT_RELU6, 1))
    finish(ctx, guards)


# ---------------------------------------------------------------------------------------------------------------- copy2d
def copy_block(guards, rows, cols, ldd, lds, seed):
    src = TC.seeded(37, rows, cols, seed).standard_normal((rows, cols), dtype=F32)
    src[0, 0], src[-1, -1] = (-0.0, 2.0 ** -140) if rows * cols > 1 else (-0.0, -0.0)
    return src, guards.inp(src, ld=lds), guards.out((rows, cols), ld=ldd)


@pytest.mark.parametrize("rows,cols,ldd,lds", TC.COPY_BLOCKS)
def test_copy2d_edges(ctx, guards, rows, cols, ldd, lds):
    src, sb, dst = copy_block(guards, rows, cols, ldd, lds, 0)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_copy2d", dst, ldd, sb, lds, rows, cols))
    assert kernels == {"copy2d_kernel": 1}
    assert same_bits(dst.download(), src)
    finish(ctx, guards)


@pytest.mark.parametrize("blocks", [TC.COPY_BLOCKS, TC.COPY_BLOCKS[2:3], [(1, 1, 1, 1), (3, 7, 9, 8), (1, 200, 200, 256)]],
                         ids=("mixed", "one", "below-256"))
def test_copy2d_batch_edges(ctx, guards, blocks):
    made = [copy_block(guards, *blk, seed=k) for k, blk in enumerate(blocks)]
    table = np.array([[dst.ptr, ldd, sb.ptr, lds, rows, cols] for (_, sb, dst), (rows, cols, ldd, lds) in zip(made, blocks)], np.int64)
    sizes = [rows * cols for rows, cols, _, _ in blocks]
    tb = guards.inp(table)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_copy2d_batch", tb, len(blocks), max(sizes), sum(sizes)))
    assert kernels == {"copy2d_batch_kernel": 1}
    for (src, sb, dst), (rows, cols, ldd, lds) in zip(made, blocks):     # == the one-by-one results, bit for bit
        single = guards.out((rows, cols), ld=ldd)
        ctx.call("ssdseg_copy2d", single, ldd, sb, lds, rows, cols)
        assert same_bits(dst.download(), single.download()) and same_bits(dst.download(), src)
    finish(ctx, guards)


# ---------------------------------------------------------------------------------------------------- argument contracts
def test_argument_contracts(ctx, guards):
    """every call is rejected with the library's argument error before anything is launched: the outputs stay poison"""
    from ssdseglib import _hip as H
    x = guards.inp(TC.seeded(38).standard_normal((16, 8), dtype=F32))
    s4 = guards.inp(np.ones(8, F32))
    out = guards.out((16, 8))
    small = guards.out(4)
    w = c4(TC.CW)

    def calls():
        rejected(ctx, "ssdseg_channel_shuffle", H.view(x), 8, x, 8, 16, 8, 2, 0)                  # out == in->x
        rejected(ctx, "ssdseg_channel_shuffle", H.view(x), 8, out, 8, 16, 8, 3, 0)                # c % groups != 0
        rejected(ctx, "ssdseg_channel_shuffle", H.view(x), 8, out, 7, 16, 8, 2, 0)                # ldo < c
        rejected(ctx, "ssdseg_head_gather", H.view(x), out, 2, 32, 8, 2, 64, 0)                   # offset not a multiple of 4 (it fits)
        rejected(ctx, "ssdseg_head_gather", H.view(x), out, 2, 62, 8, 0, 64, 0)                   # size not a multiple of 4
        rejected(ctx, "ssdseg_head_gather", H.view(x), out, 2, 32, 8, 36, 64, 0)                  # out_img_elems < off + in_img_elems
        rejected(ctx, "ssdseg_softmax_rows", H.view(x), out, 16, 8)                               # c != 4
        rejected(ctx, "ssdseg_metric_label_accuracy", x, x, 2, 8, 8, w, small)
        rejected(ctx, "ssdseg_dice_loss", x, x, 2, 8, 8, w, 0, small)
        rejected(ctx, "ssdseg_metric_mask_iou", x, 2, 2, 4, 8, 1, 1, 0, x, w, small)
        rejected(ctx, "ssdseg_metric_mask_iou", x, 1, 1, 1, 4, 2, 2, 0, x, w, small)              # fy > 1 without from_logits
        rejected(ctx, "ssdseg_softmax_rows", H.view(x, s4, None), out, 16, 4)                     # a view with only a scale
        rejected(ctx, "ssdseg_channel_shuffle", H.view(x, None, s4), 8, out, 8, 16, 8, 2, 0)      # ... only a shift
        rejected(ctx, "ssdseg_gap_fwd", H.view(x, s4, None), out, 1, 16, 8)
        rejected(ctx, "ssdseg_copy2d", out, 32768, x, 32768, 65536, 32768)                        # rows * cols = 2^31: int overflow in the kernel
        rejected(ctx, "ssdseg_copy2d", out, 65472, x, 65472, 32768, 65472)                        # 2^31 - 2^21: the last grid step would overflow
        rejected(ctx, "ssdseg_copy2d_batch", x, 1, 2 ** 31 - 4096, 16)                            # the same for a row of the batch table
        rejected(ctx, "ssdseg_dice_loss", x, x, 65536, 1, 4, w, 0, small)                         # n is gridDim.y
        rejected(ctx, "ssdseg_metric_mask_iou", x, 65536, 1, 1, 4, 1, 1, 0, x, w, small)
    assert launched(ctx, calls) == {}
    assert untouched(out) == 16 * 8 and untouched(small) == 4
    finish(ctx, guards)
