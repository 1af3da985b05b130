"""The cases, references and bounds of tests/_tail_cases.py, vetted on the CPU alone (no GPU, no library).

New references agree with an independent formulation (torch on the CPU where it has the operation); every named case has the
property it is named for, asserted on the float64 reference, so that a changed seed cannot empty it; every reduction bound is tight
enough that a structural error (a partial block, a chunk or a pixel dropped or repeated) moves the reference by at least ten times
the bound.  The structural unit is the one the launch of the case has: a partial block where there is more than one, a chunk where
the pixel sum is split, otherwise a pixel.  Every block is seen; of the single pixels and chunks at least 90 %: a unit whose own ratio
is the image's (dice, Jaccard), or that sums to nothing (pixel sums), moves the value by nothing whatever the bound.  One property
the reference does not have: a predicted extent clamped at 0 cannot change metric_box_iou (an intersection extent is at most either
box's extent, so such a row has I = 0 with or without the clamp); test_box_cases asserts that instead.
"""
import numpy as np
import pytest
import torch

import _tail_cases as TC
from oracle import np_ops as O

F32 = np.float32


# ------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("m,c,groups", TC.SHUFFLE_SHAPES[:4])
def test_shuffle_reference_and_index(m, c, groups):
    x = TC.seeded(20, m, c).normal(0, 1, (m, c)).astype(F32)
    want = torch.from_numpy(x).reshape(m, groups, c // groups).permute(0, 2, 1).reshape(m, c).numpy()
    assert np.array_equal(TC.shuffle_ref(x, groups), want)
    assert np.array_equal(x[:, TC.shuffle_index(c, groups)], want)
    assert np.array_equal(TC.shuffle_ref(want, groups, inverse=True), x)
    assert np.array_equal(want[:, TC.shuffle_index(c, groups, inverse=True)], x)


@pytest.mark.parametrize("name", list(TC.gather_tables()))
def test_gather_reference(name):
    ldi, table = TC.gather_tables()[name]
    assert table.min() >= -1 and table.max() < ldi          # an out-of-range entry is a caller error and is never tried
    x = TC.seeded(21, ldi).normal(0, 2, (5, ldi)).astype(F32)
    s, t = TC.gather_view_params(ldi, 3)
    base = TC.seeded(22, ldi).normal(0, 1, (5, table.size))
    got, mag = TC.channel_gather_ref(x, table, s, t, O.ACT_RELU6, base)
    tx = torch.from_numpy(x.astype(np.float64))
    act = torch.clamp(tx * torch.from_numpy(s.astype(np.float64)) + torch.from_numpy(t.astype(np.float64)), 0, 6)
    live = torch.from_numpy(table >= 0)
    want = torch.index_select(act, 1, torch.from_numpy(np.where(table >= 0, table, 0).astype(np.int64))) * live + torch.from_numpy(base)
    assert np.abs(got - want.numpy()).max() < 1e-12
    pad = table < 0
    if pad.any():       # a padding entry is 0 (the base under accumulate), never act(shift)
        assert np.array_equal(got[:, pad], base[:, pad]) and not mag[:, pad].any()
        plain, _ = TC.channel_gather_ref(x, table, s, t, O.ACT_RELU6)
        assert not plain[:, pad].any()
        assert (O.act_fwd(t.astype(np.float64), O.ACT_RELU6) != 0).all()


def test_split_tables_are_the_products():
    (f0, c0, b0), (f1, c1, b1) = TC.split_tables()
    assert c0 == c1 == 60 and (f0[58:] == -1).all() and (f1[58:] == -1).all()
    assert np.array_equal(f0[:58], np.arange(58)) and np.array_equal(f1[:58], np.arange(58, 116))
    packed = np.arange(116.0)[None]
    back = TC.channel_gather_ref(TC.channel_gather_ref(packed, f0)[0], b0)[0] + TC.channel_gather_ref(TC.channel_gather_ref(packed, f1)[0], b1)[0]
    assert np.array_equal(back, packed)


def test_head_gather_reference():
    b, cells, c, off, total = TC.GATHER_SHAPES[1]
    x = TC.seeded(23).normal(0, 2, (b, cells, c)).astype(F32)
    s, t = TC.view_params(c, 1)
    ref, written, mag = TC.head_gather_ref(x, s, t, O.ACT_RELU, off, total)
    flat = torch.relu(torch.from_numpy(x.astype(np.float64)) * torch.from_numpy(s.astype(np.float64)) + torch.from_numpy(t.astype(np.float64)))
    want = torch.zeros(b, total * 4, dtype=torch.float64)
    want[:, off * 4:off * 4 + cells * c] = flat.reshape(b, -1)
    assert np.abs(ref.reshape(b, -1) - want.numpy()).max() < 1e-12
    assert written.reshape(b, -1).sum(1).tolist() == [cells * c] * b and not mag[~written].any()
    assert len({tuple(r) for r in s.reshape(-1, 4)}) > 1       # the channel of an element matters: c > 4


def test_copy2d_reference():
    rng = TC.seeded(24)
    dst, src = rng.normal(0, 1, (5, 9)), rng.normal(0, 1, (6, 12))
    out = TC.copy2d_ref(dst, src, 4, 7)
    want = torch.from_numpy(dst).clone()
    want[:4, :7] = torch.from_numpy(src)[:4, :7]
    assert np.array_equal(out, want.numpy()) and np.array_equal(out[4:], dst[4:]) and np.array_equal(out[:, 7:], dst[:, 7:])


def test_softmax_and_mean_references():
    z = TC.softmax_case(257, 30.0)
    assert np.abs(TC.softmax_ref(z) - torch.softmax(torch.from_numpy(z.astype(np.float64)), -1).numpy()).max() < 1e-15
    x = TC.gap_case(2, 63, 12)
    assert np.abs(O.gap_fwd(x.astype(np.float64)[:, :, None])[:, 0, 0] - torch.from_numpy(x.astype(np.float64)).mean(1).numpy()).max() < 1e-14


def test_mode2_reference_is_the_cross_entropy():
    y, p = TC.dice_case(2, 255)
    want, _ = O.cross_entropy_loss(y[:, :, None], p[:, :, None], np.asarray(TC.CW, F32))
    assert np.abs(TC.dice_ref(y, p, TC.CW, 2) - want).max() < 1e-4 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------- launch mirrors
def test_launch_mirrors():
    assert [TC.pixel_sum_launch(*s)["chunks"] for s in TC.GAP_SHAPES] == TC.GAP_CHUNKS
    la = TC.pixel_sum_launch(1, 1024, 516)
    assert (la["bx"], la["gy"]) == (128, 2)                  # cv = 129: a second grid column with one live lane
    assert TC.pixel_sum_launch(2, 63, 12)["by"] == 63 and TC.pixel_sum_launch(1, 1, 4)["by"] == 1      # by capped by hw
    assert TC.pixel_sum_launch(2, 4, 8)["one_launch"] and not TC.pixel_sum_launch(2, 4, 8, accumulate=1)["one_launch"]
    assert not TC.pixel_sum_launch(2, 4, 8, pitched_out=True)["one_launch"]
    assert [TC.pixel_sum_launch(n, fy * fx, c)["chunks"] for n, c, fy, fx in TC.BILINEAR_1X1_SHAPES] == [1, 1, 16]
    assert [TC.dice_launch(hw)["nblk"] for _, hw in TC.DICE_SHAPES] == [1, 1, 1, 1, 2, 3, 64, 64, 1]
    assert TC.dice_launch(133121)["trips"] == 9 and TC.dice_launch(131072)["trips"] == 8
    assert [TC.iou_launch(h * w)["nblk"] for _, h, w in TC.IOU_PROB_SHAPES] == [1, 1, 1, 2, 64, 64, 1]
    for work in (2 * 1048580, TC.SOFTMAX_ROWS[-1], 4100 * 512, 9100 * 232, 18079 * 116, 2050 * 1024):
        assert work > TC.SECOND_TRIP                          # the second grid-stride trip


# ------------------------------------------------------------------------------------------------- case properties
def structural_errors_seen(value_of, ref, bound, npix, nblk):
    """value_of(pixel indices) with every partial block in turn (every pixel where there is one block) lost and counted twice:
    True when the value moves by at least 10 x bound -- for every block; for 90 % of the single pixels (a pixel whose own ratio is
    the image's moves a ratio of sums by nothing, whatever the bound)"""
    everything = np.arange(npix)
    units = [np.flatnonzero((everything // 256) % nblk == q) for q in range(nblk)] if nblk > 1 else [np.array([j]) for j in range(npix)]
    seen = []
    for unit in units:
        for idx in (np.delete(everything, unit), np.concatenate([everything, unit])):
            seen.append(np.abs(value_of(idx) - ref) >= 10 * bound)
    seen = np.array(seen)
    return seen.all() if nblk > 1 else seen.mean() > 0.9


def test_dice_cases_have_their_properties():
    y, p = TC.dice_case(3, 4100, "absent")
    assert not y[0, :, 3].any() and not p[0, :, 3].any() and y[1, :, 3].any()
    for mode in (0, 1):     # the absent class: (0 + e) / (0 + e) = 1, its term exactly 0 -- with nothing but that class weighted
        only3 = (0.0, 0.0, 0.0, 1.0)
        assert TC.dice_ref(y, p, only3, mode)[0] == 0.0 and TC.dice_ref(y, p, only3, mode)[1] != 0.0
    y, p = TC.dice_case(2, 40, "clip")
    assert set(np.unique(p)) == set(TC.CLIP_EDGES.tolist()) and (y[p == 0] > 0).any() and (y[p == 1] > 0).any()
    clipped = np.clip(p, TC.LO32, TC.HI32)
    assert (clipped != p).any() and (clipped == p).any()
    assert np.isfinite(TC.dice_ref(y, p, TC.CW, 2)).all()


@pytest.mark.parametrize("n,hw", TC.DICE_SHAPES)
@pytest.mark.parametrize("mode", TC.DICE_MODES)
def test_dice_bound_catches_a_structural_error(n, hw, mode):
    y, p = TC.dice_case(n, hw)
    ref, bound = TC.dice_ref(y, p, TC.CW, mode), TC.dice_bound(y, p, TC.CW, mode)
    assert (bound > 0).all() and (bound < 1e-4 * np.maximum(np.abs(ref), 1e-3)).all()
    if hw > 1:
        assert structural_errors_seen(lambda idx: TC.dice_ref(y[:, idx], p[:, idx], TC.CW, mode), ref, bound, hw, TC.dice_launch(hw)["nblk"])


@pytest.mark.parametrize("n,h,w", TC.IOU_PROB_SHAPES)
def test_iou_cases_and_bound(n, h, w):
    y, p = TC.iou_prob_case(n, h, w)
    npix = h * w
    assert not y[0, 0].any()                                # a pixel without any class
    if npix >= 8:
        assert not y[0, :, 2].any()                         # a class absent from y: its term is exactly 0
        assert TC.iou_ref(y, p, (0, 0, 1, 0))[0] == 0.0
    assert TC.iou_ref(y, p, TC.CW_ZERO)[0] != TC.iou_ref(y, p, TC.CW)[0] or npix == 1
    ref, bound = TC.iou_ref(y, p, TC.CW), TC.iou_bound(y, p, TC.CW)
    assert (bound < 1e-4 * np.maximum(ref, 1e-3)).all()
    if npix < 8:
        return
    assert structural_errors_seen(lambda idx: TC.iou_ref(y[:, idx], p[:, idx], TC.CW), ref, bound, npix, TC.iou_launch(npix)["nblk"])


def test_iou_logit_cases():
    for shape in TC.IOU_LOGIT_SHAPES:
        y, logits, p = TC.iou_logit_case(*shape)
        assert np.abs(logits).max() <= TC.LOGIT_MAG and np.abs(p.sum(-1) - 1).max() < 1e-12
        assert shape[3] & (shape[3] - 1) == 0 and shape[4] & (shape[4] - 1) == 0       # exact blend fractions (logits_prob_error)
        bound = TC.iou_bound(y, p, TC.CW, TC.logits_prob_error(TC.LOGIT_MAG))
        assert (bound < 1e-4).all()


@pytest.mark.parametrize("b,a", TC.ACC_SHAPES)
def test_accuracy_cases(b, a):
    t, p, ties = TC.accuracy_case(b, a)
    first, last = TC.accuracy_counts(t, p), TC.accuracy_counts(t, p, last=True)
    for k in ties:          # every tie row alone changes the counts when the first maximum is replaced by the last
        assert (TC.accuracy_counts(t[:, k:k + 1], p[:, k:k + 1]) != TC.accuracy_counts(t[:, k:k + 1], p[:, k:k + 1], last=True)).any()
    assert (first != last).any()
    for w in (TC.LW, TC.CW):
        ref = TC.accuracy_ref(t, p, w)
        assert np.abs(ref - (first / a * TC.w64(w)).sum(-1)).max() < 1e-15
        assert np.abs(ref - (last / a * TC.w64(w)).sum(-1)).min() > 10 * TC.accuracy_bound(t, p, w).max()
    if a > 1:
        assert not t[:, 3].any() and np.signbit(t[:, 5]).all() and t[0, 4].tolist() == [0.5, 0.5, 0, 0]


@pytest.mark.parametrize("a", TC.BOX_SIZES)
def test_box_cases(a):
    t, p, anchors, kind = TC.box_case(a)
    ref = TC.box_ref(t, p, anchors)
    terms = TC.box_terms(t, p, anchors)
    assert np.isnan(ref[0]) and np.isfinite(ref[1:]).all()
    assert terms["nb"].sum(-1).tolist()[:3] == [0, 1, a]
    assert (np.abs(p[..., 2:].astype(np.float64) * 0.2) <= 1.2 + 1e-6).all() and (np.abs(t[..., 2:] * 0.2) <= 1.2).all()
    live = terms["nb"] > 0
    assert (terms["den"][live] > 1.0).all() and (terms["e_den"][live] < 1e-3 * terms["den"][live]).all()     # away from epsilon
    bound = TC.box_bound(t, p, anchors)
    assert (bound[1:] < 1e-3).all()
    e = 3
    if (kind == 0).any():   # perfect prediction: q = A / (A + e), below 1
        q = terms["q"][e, kind == 0]
        assert (q < 1).all() and (q > 1 - 1e-6).all()
    if (kind == 1).any():   # the denormal offset is an object
        assert (terms["nb"][e, kind == 1] == 1).all()
        assert abs(TC.box_ref(t, p, anchors, denormal_is_object=False)[e] - ref[e]) > 10 * bound[e]
    if (kind == 2).any():
        assert (terms["nb"][e, kind == 2] == 0).all() and np.signbit(t[e, kind == 2, 0]).all()
    if (kind == 3).any():   # predicted extents clamped at 0: the areas change with the clamp, the value cannot (I <= either extent)
        free = TC.box_terms(t, p, anchors, clamp=False)
        assert (free["den"][e, kind == 3] != terms["den"][e, kind == 3]).all()
        assert not terms["q"][e, kind == 3].any() and not free["q"][e, kind == 3].any()
    if (kind == 4).any():   # touching boxes: the +1 extent is what makes them overlap
        assert (terms["inter"][e, kind == 4] > 0).all()
        assert (TC.box_terms(t, p, anchors, plus_one=0.0)["inter"][e, kind == 4] == 0).all()
        assert abs(TC.box_ref(t, p, anchors, plus_one=0.0)[e] - ref[e]) > 10 * bound[e]
    if (kind == 5).any():
        assert (terms["inter"][e, kind == 5] == 0).all()
    if 1 < a <= 257:        # every anchor in turn dropped, and counted twice, in the image whose anchors are all objects
        q = terms["q"][2]
        moved = np.abs(np.concatenate([(q.sum() - q) / (a - 1), (q.sum() + q) / (a + 1)]) - ref[2])
        assert (moved >= 10 * bound[2]).mean() > 0.9        # (an anchor whose quotient is the image's mean moves the mean by nothing)
    # a = 9600 is not held to this: the value is a mean, the bound is the mean of the per-anchor decode errors (3e-5 of the value,
    # whatever a) and one anchor weighs 1e-4 of it.  The loop is the one a = 257 runs with two trips; here it runs 38.
    assert a <= 257 or (bound[2] / ref[2] > 1e-5 and 1.0 / a < 2e-4)


def test_softmax_cases():
    for spread in TC.SOFTMAX_SPREADS:
        z = TC.softmax_case(257, spread)
        ref = TC.softmax_ref(z)
        assert (ref[0] == 0.25).all() and np.abs(ref.sum(-1) - 1).max() < 1e-15
        assert (TC.softmax_bound(z) < 300 * TC.U).all()
    ref = TC.softmax_ref(TC.softmax_case(257, 200.0))
    assert ref[1, 0] == 1.0 and 0 < ref[1, 3] < 2.0 ** -149 and 0 < ref[1, 2] < TC.TINY      # the smallest terms underflow in float32
    big = TC.softmax_case(257, 1.0, offset=1e30)
    assert np.isfinite(big).all() and (big > 9e29).all() and np.isfinite(TC.softmax_ref(big)).all()


@pytest.mark.parametrize("n,hw,c", TC.GAP_SHAPES)
def test_gap_bound_catches_a_structural_error(n, hw, c):
    x = TC.gap_case(n, hw, c)
    s, t = TC.view_params(c, 2)
    la = TC.pixel_sum_launch(n, hw, c)
    for scale, shift, act in ((None, None, O.ACT_NONE), (s, t, O.ACT_RELU6)):
        a, _ = TC.view_ref(x, scale, shift, act)
        ref, bound = a.mean(1), TC.pixel_sum_bound(a, la, 3) / hw
        assert np.abs(ref - O.gap_fwd(a[:, :, None])[:, 0, 0]).max() < 1e-14
        if hw == 1:
            continue
        # every chunk (every pixel where the sum is not split) in turn: what it moves, per channel -- by -unit / hw when it is lost,
        # by +unit / hw when it is counted twice, so one magnitude answers for both
        units = a.reshape(n, la["chunks"], la["hwc"], c).sum(2) if la["chunks"] > 1 else a
        moved = np.abs(units) / hw
        seen = moved[moved > 0] >= 10 * np.broadcast_to(bound[:, None], moved.shape)[moved > 0]
        # (a unit that sums to almost nothing proves nothing either way.)  (600, 1024, 4) has one channel vector, so row 0 of its block
        # folds 512 partial sums in one thread: the worst-case chain is 518 roundings, 3e-5 of the sum, and a pixel is 1e-3 of it --
        # only the pixels above a third of the mean magnitude stand 10 x clear of that
        assert seen.mean() > (0.75 if la["by"] == 512 else 0.98) and (bound < 1e-4).all()
