"""ssdseg_eval_mask_scores (csrc/evaluate.hip) and evaluate_on_device's `ignore_void` / `confusion` options on the GPU.

1. The kernel on the cases of tests/_void_cases.py (probabilities that are ratios of small integers, with exact ties between classes,
   class indices >= c and 255, an all-void last image): c = 4 on the dword / float4 path with n in {1, 3}, hw in {1, 7, 1030, 4101} and the class
   indices 0..3 bytes off a dword boundary (heads and tails of every length, several blocks per image), and c = 3, c = 8 on the
   general path.  The confusion and void counts equal the reference (np.argmax) exactly, two runs give the same bytes, with
   ignore_void = 0 the Jaccard output has the bits of ssdseg_eval_mask_jaccard, with ignore_void = 1 it is within the bound
   tests/test_gpu_evaluate.py takes for the Jaccard against float64 (2e-4) of the labelled-only reference.
2. evaluate_on_device(confusion=True, ignore_void=True) on the small trained model of tests/test_gpu_evaluate.py, two compact
   batches of different size: 'confusion' is confusion_matrix_semantic_segmentation on predict's masks, the scores are
   scores_from_confusion of it, 'ap' and 'detections' are those of the call without the options.
"""
import numpy as np
import pytest

import _void_cases as VC
from tests.test_gpu_evaluate import (BACKGROUND, B_THRESHOLD, JACCARD_TOL, LABELS_CODES, P_THRESHOLD, compact_batches, inference_model, predict_batches,
                                     trained)  # noqa: F401  (trained: fixture)
from _guard import guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_scores(ctx, guards, prob, index, c, mask_off, ignore_void, want=("iou", "confusion", "void")):
    """-> {name: array} of one ssdseg_eval_mask_scores call on guarded buffers, the class indices mask_off bytes into theirs"""
    n, hw = index.shape
    d_prob = guards.inp(prob)
    d_index = guards.inp(np.concatenate([np.zeros(mask_off, np.uint8), index.ravel()]))
    outs = dict(iou=guards.out((n, c)), confusion=guards.out((n, c, c), np.int32), void=guards.out(n, np.int32))
    args = [outs[k] if k in want else None for k in ("iou", "confusion", "void")]
    ctx.call("ssdseg_eval_mask_scores", d_prob, d_index.view(mask_off, (n, hw)), n, hw, c, ignore_void, *args)
    got = {k: outs[k].download() for k in want}
    for k in ("iou", "confusion", "void"):
        assert len(guards.unwritten(outs[k])) == (0 if k in want else outs[k].size), k
    return got, (d_prob, d_index.view(mask_off, (n, hw)))


def check_scores(ctx, guards, n, hw, c, mask_off):
    prob, index = VC.eval_case(n, hw, c)
    want_m, want_void = VC.confusion_ref(prob, index, c)
    ties = int((np.sort(prob, -1)[..., -1] == np.sort(prob, -1)[..., -2]).sum()) if c > 1 else 0
    assert (hw < 7 or (ties > 0 and (index >= c).any())) and (n == 1 or want_void[-1] == hw)
    for ignore_void in (0, 1):
        first, (d_prob, d_index) = run_scores(ctx, guards, prob, index, c, mask_off, ignore_void)
        again, _ = run_scores(ctx, guards, prob, index, c, mask_off, ignore_void)
        assert np.array_equal(first["confusion"], want_m) and np.array_equal(first["void"], want_void)
        assert first["confusion"].sum() + first["void"].sum() == n * hw
        for k in first:
            assert np.array_equal(bits(first[k]), bits(again[k])), f"{k}: two runs, two results"
        if ignore_void == 0:
            plain = guards.out((n, c))
            ctx.call("ssdseg_eval_mask_jaccard", d_prob, d_index, n, hw, c, plain)
            assert np.array_equal(bits(first["iou"]), bits(plain.download())), "ignore_void = 0: not the bits of ssdseg_eval_mask_jaccard"
            alone, _ = run_scores(ctx, guards, prob, index, c, mask_off, 0, want=("iou",))
            assert np.array_equal(bits(alone["iou"]), bits(plain.download()))
        err = float(np.abs(first["iou"].astype(np.float64) - VC.jaccard_ref(prob, index, c, bool(ignore_void))).max())
        print(f"scores n{n} hw{hw} c{c} mask+{mask_off} ignore_void={ignore_void}: max |iou - float64| = {err:.3e}, ties {ties}")
        assert err < JACCARD_TOL
        if n > 1 and ignore_void:
            assert not first["iou"][-1].any()                              # an all-void image: I = T = 0
        only, _ = run_scores(ctx, guards, prob, index, c, mask_off, ignore_void, want=("confusion",))
        assert np.array_equal(only["confusion"], want_m)


@pytest.mark.parametrize("mask_off", (0, 1, 2, 3))
@pytest.mark.parametrize("hw", (1, 7, 1030, 4101))
@pytest.mark.parametrize("n", (1, 3))
def test_mask_scores_c4(ctx, guards, n, hw, mask_off):
    check_scores(ctx, guards, n, hw, 4, mask_off)


@pytest.mark.parametrize("c", (3, 8))
@pytest.mark.parametrize("n,hw", [(1, 7), (3, 1030)])
def test_mask_scores_general_path(ctx, guards, n, hw, c):
    check_scores(ctx, guards, n, hw, c, 1)


def test_mask_scores_rejects_bad_arguments(ctx, guards):
    from ssdseglib._hip import SsdsegError
    prob, index = guards.inp(np.full((1, 4, 4), 0.25, np.float32)), guards.inp(np.zeros((1, 4), np.uint8))
    iou, conf, void = guards.out((1, 4)), guards.out((1, 4, 4), np.int32), guards.out(1, np.int32)
    for args, code in (((prob, index, 1, 4, 0, 0, iou, conf, void), -1006), ((prob, index, 1, 4, 9, 0, iou, conf, void), -1006),
                       ((prob, index, 0, 4, 4, 0, iou, conf, void), -1004), ((prob, index, 65536, 4, 4, 0, iou, conf, void), -1004),
                       ((prob, index, 1, 0, 4, 0, iou, conf, void), -1005), ((prob, index, 1, 1 << 28, 4, 0, iou, conf, void), -1005),
                       ((prob, None, 1, 4, 4, 0, iou, conf, void), -1003), ((prob, index, 1, 4, 4, 1, None, None, None), -1008)):
        with pytest.raises(SsdsegError, match=str(code)):
            ctx.call("ssdseg_eval_mask_scores", *args)
    ctx.call("ssdseg_eval_mask_scores", prob, index, 1, 4, 4, 1, iou, conf, void)
    assert conf.download()[0, 0, 0] == 4 and void.download()[0] == 0 and len(guards.unwritten(iou)) == 0


def test_evaluate_on_device_confusion_and_void(ctx, guards, trained):
    from ssdseglib import _engine as E, evaluators
    E.set_default_context(ctx)
    model = inference_model(trained, True)
    seg, _ = predict_batches(model, trained)
    index = trained["index"]
    assert (index >= 4).any()
    plain = evaluators.evaluate_on_device(model, compact_batches(trained), LABELS_CODES, BACKGROUND, [0.5])
    got = evaluators.evaluate_on_device(model, compact_batches(trained), LABELS_CODES, BACKGROUND, [0.5], confusion=True, ignore_void=True)
    assert set(plain) == {"iou", "ap", "detections"}
    assert set(got) == {"iou", "ap", "detections", "confusion", "void_pixels", "iou_hard", "miou", "pixel_accuracy"}
    want_m, want_void = evaluators.confusion_matrix_semantic_segmentation(seg, index, 4)
    assert np.array_equal(got["confusion"], want_m) and got["confusion"].dtype == np.int64 and got["void_pixels"] == want_void > 0
    iou_hard, miou, acc = evaluators.scores_from_confusion(want_m, LABELS_CODES)
    print(f"miou {miou!r} pixel accuracy {acc!r} iou_hard {iou_hard}")
    assert got["iou_hard"].keys() == iou_hard.keys() and list(got["iou_hard"]) == LABELS_CODES
    assert all(got["iou_hard"][l] == iou_hard[l] or (np.isnan(got["iou_hard"][l]) and np.isnan(iou_hard[l])) for l in iou_hard)
    assert (got["miou"] == miou or (np.isnan(miou) and np.isnan(got["miou"]))) and got["pixel_accuracy"] == acc
    pair = (B_THRESHOLD, P_THRESHOLD)
    assert np.array_equal(bits(got["detections"][pair]), bits(plain["detections"][pair])) and got["ap"] == plain["ap"]
    n = seg.shape[0]
    want_iou = VC.jaccard_ref(seg.reshape(n, -1, 4), index.reshape(n, -1), 4, True).mean(axis=0)
    for l in (1, 2, 3):
        assert abs(got["iou"][l] - want_iou[l]) < JACCARD_TOL
    only = evaluators.evaluate_on_device(model, compact_batches(trained), LABELS_CODES, BACKGROUND, [0.5], confusion=True)
    assert only["iou"] == plain["iou"] and np.array_equal(only["confusion"], want_m)      # ignore_void off: the plain Jaccard's bits
