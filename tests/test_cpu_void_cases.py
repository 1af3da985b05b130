"""The void-pixel references and the confusion matrix without a GPU (tests/_void_cases.py, ssdseglib.evaluators), and the bindings
of the `ignore_void` options.

1. With nothing void the references are the plain ones: dice and Jaccard against oracle.np_ops (through tests/_mask_cases.py /
   tests/_tail_cases.py), the bootstrapped loss against tests/_bootstrap_oracle.py.
2. Central finite differences of the float64 dice and bootstrapped references confirm the stated gradients, zero rows at void
   pixels included.
3. keep_i at L = 0, 1, 3, 4, 5 for keep_fraction 0.25 / 1.0 / 1e-9; an image without a labelled pixel.
4. The confusion reference: arg-max ties go to the lowest index, an index >= C is void; scores_from_confusion gives NaN for an
   absent class and leaves it out of the mean.
5. Bindings on the recording stub of tests/test_cpu_loss_bindings.py: ignore_void=False binds today's entries with today's
   arguments, True the _void ones; values that are no bool raise.
6. evaluate_on_device with the options off: today's calls, today's key set; with them on: the scores path and the new keys.
"""
import numpy as np
import pytest

import _bootstrap_oracle as B
import _mask_cases as MC
import _tail_cases as TC
import _void_cases as VC
from oracle import np_ops as O
from ssdseglib import evaluators
from ssdseglib import losses as LS
from ssdseglib import metrics as MT
from tests.test_cpu_loss_bindings import BATCH, CW, PIXELS, bind, check_call, head_args, step, stub_engine

SHAPE = (2, 3, 5, 2, 2)


# ------------------------------------------------------------------------------------------ 1. nothing void: the plain references
@pytest.mark.parametrize("squared", (0, 1))
def test_dice_reference_without_void_is_the_plain_one(squared):
    case = VC.void_case(SHAPE, "none")
    y, p = case["y"], case["p"]
    loss, coef = VC.dice_void_ref(y, p, VC.CW, squared)
    loss_plain, coef_plain = MC.dice_ref(y, p, VC.CW, squared)
    assert np.array_equal(loss, loss_plain) and np.array_equal(coef, coef_plain)
    want = O.dice_loss(y.astype(np.float64)[:, :, None], p[:, :, None], VC.w64(VC.CW), squared=bool(squared))
    assert np.allclose(loss, want, rtol=1e-9, atol=0)                      # (the oracle's epsilon is 1e-7, the device's float32(1e-7))
    assert np.array_equal(VC.dice_void_dp(y, p, coef, squared), MC.dice_dp(y, p, coef, squared))
    ref, bound = VC.dice_void_backward(case, VC.CW, squared, 0.5)
    ref_plain, bound_plain = MC.dice_backward(case, VC.CW, squared, 0.5)
    assert np.array_equal(ref, ref_plain) and np.array_equal(bound, bound_plain)
    assert np.array_equal(VC.dice_void_bound(case, VC.CW, squared), MC.dice_bound(y, p, case["bp"], VC.CW, squared))


def test_jaccard_reference_without_void_is_the_plain_one():
    case = VC.void_case(SHAPE, "none")
    y, p = case["y"], case["p"]
    assert np.allclose(VC.iou_void_ref(y, p, VC.CW), TC.iou_ref(y, p, VC.CW), rtol=1e-9, atol=0)
    assert np.array_equal(VC.iou_void_bound(y, p, VC.CW, 1e-6), TC.iou_bound(y, p, VC.CW, 1e-6))
    prob, index = VC.eval_case(2, 50, 4)
    index = index % 4                                                      # every pixel labelled
    assert np.array_equal(VC.jaccard_ref(prob, index, 4, True), VC.jaccard_ref(prob, index, 4, False))


@pytest.mark.parametrize("fraction", VC.KEEP_FRACTIONS)
def test_bootstrapped_reference_without_void_is_the_plain_one(fraction):
    case = VC.void_case(SHAPE, "none")
    y, p = case["y"], case["p"]
    npix = y.shape[1]
    got = VC.bootstrap_void_ref(y, p, VC.CW, fraction)
    keep = B.keep_count(fraction, npix)
    assert (got["keep"] == keep).all()
    n, h, w, fy, fx = SHAPE
    image = (n, h * fy, w * fx, 4)
    loss, dp, mask, thresh = B.bootstrapped_cross_entropy(y.astype(np.float64).reshape(image), p.reshape(image), VC.w64(VC.CW), keep)
    # the oracle clips at 1e-7 / 1 - 1e-7, the restatement at the device's float32 bounds: no probability of this family is near either
    assert np.array_equal(got["mask"], mask.reshape(n, npix)) and np.allclose(got["thresh"], thresh, rtol=1e-12, atol=0)
    assert np.allclose(got["loss"], loss, rtol=1e-12, atol=0) and np.allclose(got["dp"], dp.reshape(n, npix, 4), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------------ 2. finite differences
def numeric_gradient(loss_of, p, picks, h=1e-6):
    out = np.zeros(len(picks))
    for k, idx in enumerate(picks):
        hi, lo = p.copy(), p.copy()
        hi[idx] += h
        lo[idx] -= h
        out[k] = (loss_of(hi)[idx[0]] - loss_of(lo)[idx[0]]) / (2 * h)
    return out


def picks_of(case, count=24):
    """entries of p to move: void and labelled pixels of every image; of a labelled pixel its own class or, every other time, any"""
    rng = VC.seeded(74)
    y = case["y"]
    lab = VC.labelled(y)
    picks = []
    for i in range(y.shape[0]):
        for group in (np.flatnonzero(lab[i]), np.flatnonzero(~lab[i])):
            for k, px in enumerate(rng.permutation(group)[:count // 4]):
                own = lab[i, px] and k % 2 == 0
                picks.append((i, int(px), int(y[i, px].argmax()) if own else int(rng.integers(0, 4))))
    return picks


@pytest.mark.parametrize("pattern", ("scattered", "rect", "image"))
@pytest.mark.parametrize("squared", (0, 1))
def test_dice_gradient_by_finite_differences(pattern, squared):
    case = VC.void_case(SHAPE, pattern)
    y, p = case["y"], case["p"]
    _, coef = VC.dice_void_ref(y, p, VC.CW, squared)
    dp = VC.dice_void_dp(y, p, coef, squared)
    assert not dp[~VC.labelled(y)].any()                                   # exact zero rows
    picks = picks_of(case)
    num = numeric_gradient(lambda q: VC.dice_void_ref(y, q, VC.CW, squared)[0], p, picks)
    ana = np.array([dp[idx] for idx in picks])
    assert np.allclose(num, ana, rtol=1e-5, atol=1e-9), np.abs(num - ana).max()
    void_picks = [k for k, idx in enumerate(picks) if not VC.labelled(y)[idx[:2]]]
    assert void_picks and not num[void_picks].any()                        # moving a void pixel's probabilities moves nothing


@pytest.mark.parametrize("pattern", ("scattered", "rect"))
def test_bootstrapped_gradient_by_finite_differences(pattern):
    case = VC.void_case(SHAPE, pattern)
    y, p = case["y"], case["p"]
    ref = VC.bootstrap_void_ref(y, p, VC.CW, 0.25)
    assert not ref["dp"][~ref["mask"]].any() and not (ref["mask"] & ~VC.labelled(y)).any()
    # away from the threshold the selection does not move with h
    gap = np.abs(np.where(VC.labelled(y), ref["l"], np.inf) - ref["thresh"][:, None])
    picks = [idx for idx in picks_of(case, 48) if gap[idx[:2]] > 1e-3 or not VC.labelled(y)[idx[:2]]]
    num = numeric_gradient(lambda q: VC.bootstrap_void_ref(y, q, VC.CW, 0.25)["loss"], p, picks, h=1e-7)
    ana = np.array([ref["dp"][idx] for idx in picks])
    assert np.allclose(num, ana, rtol=1e-4, atol=1e-7), np.abs(num - ana).max()
    assert any(ref["mask"][idx[:2]] and y[idx] for idx in picks) and any(not VC.labelled(y)[idx[:2]] for idx in picks)


# ------------------------------------------------------------------------------------------------------------- 3. keep_i
@pytest.mark.parametrize("fraction,want", [(0.25, [0, 1, 1, 1, 2]), (1.0, [0, 1, 3, 4, 5]), (1e-9, [0, 1, 1, 1, 1])])
def test_keep_edge_values(fraction, want):
    assert [VC.keep_void(fraction, l) for l in (0, 1, 3, 4, 5)] == want
    for l in (1, 3, 4, 5):
        assert VC.keep_void(fraction, l) == LS.bootstrap_keep(fraction, l) == B.keep_count(fraction, l)


def test_an_image_without_a_labelled_pixel():
    case = VC.void_case((2, 3, 5, 2, 2), "image")
    y, p = case["y"], case["p"]
    assert not y[1].any() and y[0].any()
    for squared in (0, 1):
        loss, coef = VC.dice_void_ref(y, p, VC.CW, squared)
        assert loss[1] == 0.0 and loss[0] != 0.0                           # (2*0 + eps) / (0 + eps) = 1
        assert not VC.dice_void_dp(y, p, coef, squared)[1].any()
    ref = VC.bootstrap_void_ref(y, p, VC.CW, 0.25)
    assert ref["loss"][1] == 0.0 and ref["kept"][1] == 0 and ref["keep"][1] == 0 and ref["thresh"][1] == np.inf
    assert not ref["dp"][1].any() and not ref["mask"][1].any()
    assert VC.iou_void_ref(y, p, VC.CW)[1] == 0.0
    single = VC.void_case((2, 3, 5, 2, 2), "single")
    ref = VC.bootstrap_void_ref(single["y"], single["p"], VC.CW, 0.25)
    assert ref["keep"].tolist() == [1, 1] and ref["kept"].tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------------------- 4. confusion
def test_confusion_reference_ties_and_void():
    prob = np.array([[[0.4, 0.4, 0.1, 0.1], [0.1, 0.2, 0.35, 0.35], [0.25, 0.25, 0.25, 0.25], [0.0, 0.0, 0.0, 1.0], [0.7, 0.1, 0.1, 0.1]]], np.float32)
    index = np.array([[1, 2, 3, 4, 255]], np.uint8)
    m, void = evaluators.confusion_matrix_semantic_segmentation(prob.reshape(1, 1, 5, 4), index.reshape(1, 1, 5), 4)
    want = np.zeros((4, 4), np.int64)
    want[1, 0] = want[2, 2] = want[3, 0] = 1                               # ties go to the lowest index
    assert np.array_equal(m, want) and m.dtype == np.int64 and void == 2 and isinstance(void, int)
    per_image, per_void = VC.confusion_ref(prob, index, 4)
    assert np.array_equal(per_image[0], want) and per_void.tolist() == [2]
    for c in (3, 4, 8):
        prob, index = VC.eval_case(3, 257, c)
        m, void = evaluators.confusion_matrix_semantic_segmentation(prob, index, c)
        per_image, per_void = VC.confusion_ref(prob, index, c)
        assert np.array_equal(m, per_image.sum(0)) and void == per_void.sum() and m.sum() + void == index.size
        assert per_void[-1] == 257 and not per_image[-1].any()             # the last image is all void
    with pytest.raises(ValueError):
        evaluators.confusion_matrix_semantic_segmentation(prob, index[:, :-1], 8)


def test_scores_from_confusion():
    m = np.array([[5, 1, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0], [0, 0, 0, 4]])
    iou, miou, acc = evaluators.scores_from_confusion(m, [0, 10, 20, 30])
    assert list(iou) == [0, 10, 20, 30]
    assert iou[0] == 5 / 8 and iou[10] == 3 / 6 and np.isnan(iou[20]) and iou[30] == 1.0
    assert miou == pytest.approx((5 / 8 + 0.5 + 1.0) / 3) and acc == 12 / 15
    iou, miou, acc = evaluators.scores_from_confusion(np.zeros((2, 2), np.int64), [0, 1])
    assert all(np.isnan(v) for v in iou.values()) and np.isnan(miou) and np.isnan(acc)
    m = np.array([[0, 3], [0, 0]])                                         # class 1 is predicted but never true: IoU 0, not NaN
    iou, miou, _ = evaluators.scores_from_confusion(m, [0, 1])
    assert iou == {0: 0.0, 1: 0.0} and miou == 0.0
    with pytest.raises(ValueError):
        evaluators.scores_from_confusion(np.zeros((2, 3)), [0, 1])


# ----------------------------------------------------------------------------------------------------------- 5. bindings
@pytest.mark.parametrize("factory,flag", [(LS.dice, 0), (LS.dice_square, 1)])
@pytest.mark.parametrize("void", (False, True))
def test_dice_bindings(factory, flag, void):
    fn = factory(CW, ignore_void=void)
    assert fn.ignore_void is void and factory(CW).ignore_void is False
    eng = bind(stub_engine(), mask=fn)
    op = eng.t.head
    coef = op.loss_impl.coef
    fwd, bwd = step(eng)
    suffix = "_void" if void else ""
    check_call(fwd, "ssdseg_mask_head_fwd_dice" + suffix, *head_args(eng), op.y_true, op.class_weights, flag, None, op.loss, coef)
    check_call(bwd, "ssdseg_mask_head_bwd_dice" + suffix, *head_args(eng), op.y_true, coef, flag, 0.5, eng.t.mask_logits.grad)


def test_bootstrapped_bindings():
    plain = bind(stub_engine(), mask=LS.bootstrapped_cross_entropy(CW, 0.3, ignore_void=False))
    op, impl = plain.t.head, plain.t.head.loss_impl
    fwd, bwd = step(plain)
    check_call(fwd, "ssdseg_mask_head_fwd_bootstrap", *head_args(plain), op.y_true, op.class_weights, impl.keep, None, impl.pixel_loss, impl.thresh,
               impl.kept, op.loss)
    check_call(bwd, "ssdseg_mask_head_bwd_bootstrap", *head_args(plain), op.y_true, op.class_weights, impl.pixel_loss, impl.thresh, 0.5,
               plain.t.mask_logits.grad)
    assert impl.keep == 58 and type(impl.keep) is int                     # no keep buffer without the option

    fn = LS.bootstrapped_cross_entropy(CW, 0.3, ignore_void=True)
    assert fn.ignore_void is True and fn.keep_fraction == 0.3
    eng = bind(stub_engine(), mask=fn)
    op, impl = eng.t.head, eng.t.head.loss_impl
    fwd, bwd = step(eng)
    check_call(fwd, "ssdseg_mask_head_fwd_bootstrap_void", *head_args(eng), op.y_true, op.class_weights, 0.3, None, impl.pixel_loss, impl.thresh,
               impl.keep, impl.kept, op.loss)
    check_call(bwd, "ssdseg_mask_head_bwd_bootstrap_void", *head_args(eng), op.y_true, op.class_weights, impl.pixel_loss, impl.thresh, 0.5,
               eng.t.mask_logits.grad)
    assert impl.keep.shape == (BATCH,) and impl.keep.dtype == np.int32 and impl.pixel_loss.shape == (BATCH, PIXELS)
    assert op.kind == "bootstrapped_cross_entropy" and op.pixel_loss is impl.pixel_loss and op.kept is impl.kept


@pytest.mark.parametrize("void", (False, True))
def test_metric_binding(void):
    from ssdseglib import _loss_bind as LB
    fn = MT.jaccard_iou_segmentation_masks(CW, ignore_void=void)
    assert fn.ignore_void is void and fn.metric_kind == "mask_iou" and MT.jaccard_iou_segmentation_masks(CW).ignore_void is False
    eng = bind(stub_engine(), mask=LS.cross_entropy(CW))
    LB.bind_metrics(eng, {"output-mask": fn})
    del eng.ctx.calls[:]
    LB.launch_metrics(eng)
    (call,) = eng.ctx.calls
    op = eng.t.head
    check_call(call, "ssdseg_metric_mask_iou" + ("_void" if void else ""), *head_args(eng), 1, op.y_true, fn._cw, eng._metrics[0][4])


@pytest.mark.parametrize("bad", (1, 0, None, "yes", 1.0, np.int32(1)))
def test_ignore_void_must_be_a_bool(bad):
    for make in (lambda: LS.dice(CW, ignore_void=bad), lambda: LS.dice_square(CW, ignore_void=bad),
                 lambda: LS.bootstrapped_cross_entropy(CW, 0.25, ignore_void=bad), lambda: MT.jaccard_iou_segmentation_masks(CW, ignore_void=bad)):
        with pytest.raises(ValueError, match="ignore_void"):
            make()
    assert not hasattr(LS.cross_entropy(CW), "ignore_void") or LS.cross_entropy(CW).ignore_void is False


# ------------------------------------------------------------------------------------------------- 6. evaluate_on_device
def canned(n=2, r=10, c=4):
    iou = np.full((n, c), 0.25, np.float32)
    per_pair = {(0.3, 0.4): (np.zeros((n, r, 6), np.float32), np.zeros((n, r), np.float32))}
    counts = (np.arange(n * c * c, dtype=np.int32).reshape(n, c, c), np.array([7, 9], np.int32))
    return iou, per_pair, counts


def test_evaluate_on_device_options(monkeypatch):
    from ssdseglib import _fit
    from tests.test_cpu_evaluate import BACKGROUND, LABELS_CODES, _compact, _small_inference_model
    model = _small_inference_model()
    calls = []

    def plain(*args):
        calls.append(("plain", args[2:]))
        return canned()[:2]

    def scores(*args):
        calls.append(("scores", args[2:]))
        iou, per_pair, counts = canned()
        return iou, per_pair, (counts if args[4] else None)

    monkeypatch.setattr(_fit, "run_evaluate", plain)
    monkeypatch.setattr(_fit, "run_evaluate_scores", scores)
    off = evaluators.evaluate_on_device(model, [_compact()], LABELS_CODES, BACKGROUND, [0.5])
    assert set(off) == {"iou", "ap", "detections"} and calls == [("plain", ([(0.3, 0.4)],))]
    del calls[:]
    void = evaluators.evaluate_on_device(model, [_compact()], LABELS_CODES, BACKGROUND, [0.5], ignore_void=True)
    assert set(void) == {"iou", "ap", "detections"} and calls == [("scores", ([(0.3, 0.4)], True, False))]
    del calls[:]
    on = evaluators.evaluate_on_device(model, [_compact(), _compact()], LABELS_CODES, BACKGROUND, [0.5], confusion=True)
    assert set(on) == {"iou", "ap", "detections", "confusion", "void_pixels", "iou_hard", "miou", "pixel_accuracy"}
    assert calls == [("scores", ([(0.3, 0.4)], False, True))] * 2
    want = 2 * canned()[2][0].astype(np.int64).sum(0)
    assert np.array_equal(on["confusion"], want) and on["confusion"].dtype == np.int64 and on["void_pixels"] == 32 and type(on["void_pixels"]) is int
    iou_hard, miou, acc = evaluators.scores_from_confusion(want, LABELS_CODES)
    assert on["iou_hard"] == iou_hard and list(on["iou_hard"]) == list(LABELS_CODES) and on["miou"] == miou and on["pixel_accuracy"] == acc
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="ignore_void"):
            evaluators.evaluate_on_device(model, [_compact()], LABELS_CODES, BACKGROUND, [0.5], ignore_void=bad)
        with pytest.raises(ValueError, match="confusion"):
            evaluators.evaluate_on_device(model, [_compact()], LABELS_CODES, BACKGROUND, [0.5], confusion=bad)
