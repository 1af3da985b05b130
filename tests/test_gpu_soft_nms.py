"""GPU parity of ssdseg_combined_nms_soft (csrc/boxes.hip) through the C-ABI, bit for bit against `layers.soft_nms_reference`.

The weight of the decay is defined as the correctly rounded float32 of a double expression (include/ssdseg.h), so the device and
NumPy agree in every bit and every assertion here is `array_equal`: competing scores in these cases are as close as one ulp, and a
tolerance would let a wrong pick through.  The cases are those of tests/_anchor_cases.py (tests/test_cpu_soft_nms.py shows on the
specification alone that they exercise the decay) at the anchor counts where the kernel can go wrong: 1, 5, 1023 and 1025 around
the 1024-thread block, 2100 for ties across a thread's stride, 9600, 14336 and 14337 on either side of the switch from scores in
LDS to scores in the workspace, and 150000, the argument bound.
"""
import numpy as np
import pytest

import _anchor_cases as AC
from _guard import guards  # noqa: F401  (fixture)
from tests.test_gpu_anchor_edges import decode_on_device
from tests.test_gpu_evaluate import (B_THRESHOLD, BACKGROUND, LABELS_CODES, NMS, P_THRESHOLD, compact_batches, inference_model,  # noqa: F401
                                     predict_batches, trained)

pytestmark = pytest.mark.gpu

LDS_ANCHORS = 14336           # NMS_SOFT_LDS_A of csrc/boxes.hip: the last anchor count whose scores live in LDS
CASES = {**AC.NMS_CASES,
         "a14336-lds": lambda: AC.nms_saturated(a=LDS_ANCHORS, max_per_class=20, max_total=50),
         "a14337-workspace": lambda: AC.nms_saturated(a=LDS_ANCHORS + 1, max_per_class=20, max_total=50)}
DECAY_DECIDES = ("saturated", "dry", "a14336-lds", "a14337-workspace")      # cases whose rows the decay changes (asserted)
EINVAL = lambda n: str(-1000 - n)


def reference(inputs, corners, iou_thr, sigma):
    from ssdseglib.layers import soft_nms_reference
    return soft_nms_reference(corners, inputs["probs"], inputs["max_per_class"], inputs["max_total"], iou_thr, inputs["score_thr"], sigma)


class Staged:
    """the inputs of one case on the device (guarded), its corners decoded there, and the soft / hard entry on them"""

    def __init__(self, ctx, guards, inputs):
        self.ctx, self.guards, self.inputs = ctx, guards, inputs
        if "corners" in inputs:
            self.d_corners = guards.inp(inputs["corners"])
        else:
            self.d_corners = decode_on_device(ctx, guards, inputs["offsets"], inputs["centroids"])
        self.corners = self.d_corners.download()
        self.d_probs = guards.inp(inputs["probs"])
        self.shape = inputs["probs"].shape

    def soft(self, iou_thr, sigma, with_valid=True):
        k, (b, a, c) = self.inputs, self.shape
        out = self.guards.out((b, k["max_total"], 6))
        valid = self.guards.out(b, np.int32) if with_valid else None
        self.ctx.call("ssdseg_combined_nms_soft", self.d_corners, self.d_probs, b, a, c, k["max_per_class"], k["max_total"], iou_thr,
                      k["score_thr"], sigma, out, valid)
        return out.download(), (valid.download() if with_valid else None)

    def hard(self):
        k, (b, a, c) = self.inputs, self.shape
        out, valid = self.guards.out((b, k["max_total"], 6)), self.guards.out(b, np.int32)
        self.ctx.call("ssdseg_combined_nms", self.d_corners, self.d_probs, b, a, c, k["max_per_class"], k["max_total"], k["iou_thr"],
                      k["score_thr"], out, valid)
        return out.download(), valid.download()


# -------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(CASES))
def test_soft_nms_parity(ctx, guards, name):
    inputs, _ = CASES[name]()
    s = Staged(ctx, guards, inputs)
    settings = [(thr, 0.5) for thr in dict.fromkeys((inputs["iou_thr"], 0.5, 1.0))]
    if name in ("saturated", "dry"):
        settings += [(thr, 0.1) for thr in dict.fromkeys((inputs["iou_thr"], 0.5, 1.0))]
    changed = 0
    for iou_thr, sigma in settings:
        out, valid = s.soft(iou_thr, sigma)
        want, want_valid = reference(inputs, s.corners, iou_thr, sigma)
        diff = np.argwhere((out != want).any(-1))
        print(f"{name} iou_thr={iou_thr} sigma={sigma}: valid {valid.tolist()}, {len(diff)} rows differ from the specification")
        assert np.array_equal(valid, want_valid), (iou_thr, sigma)
        assert np.array_equal(out, want), f"iou_thr={iou_thr} sigma={sigma}: {len(diff)} rows differ, first (image, row) = {diff[0].tolist()}"
        for i in range(out.shape[0]):
            assert not out[i, valid[i]:].any()                     # the tail is zero-filled
        if name in DECAY_DECIDES:
            changed += int((want != reference(inputs, s.corners, iou_thr, 1e30)[0]).any(-1).sum())
    if name in DECAY_DECIDES:
        print(f"{name}: {changed} rows differ from the hard NMS over the settings")
        assert changed > 0, "every row is the hard NMS's: the case does not exercise the decay"
    ctx.sync()
    guards.check()


# -------------------------------------------------------------------------------------- a huge sigma against the hard entry
@pytest.mark.parametrize("name", ["saturated", "tied", "thread-ties"])
def test_huge_sigma_gives_the_bytes_of_the_hard_entry(ctx, guards, name):
    inputs, _ = AC.NMS_CASES[name]()
    s = Staged(ctx, guards, inputs)
    out, valid = s.soft(inputs["iou_thr"], 1e30)
    hard, hard_valid = s.hard()
    assert valid.tolist() == hard_valid.tolist() and valid.max() > 0
    assert np.array_equal(out.view(np.uint32), hard.view(np.uint32))


# ------------------------------------------------------------------------------------------- reproducibility and arguments
def test_two_runs_same_bytes_and_no_valid(ctx, guards):
    inputs, _ = AC.nms_saturated()
    s = Staged(ctx, guards, inputs)
    first, valid = s.soft(0.5, 0.5)
    second, _ = s.soft(0.5, 0.5)
    third, none = s.soft(0.5, 0.5, with_valid=False)
    assert none is None and valid.min() > 0
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32)) and np.array_equal(first.view(np.uint32), third.view(np.uint32))


def test_argument_errors_launch_nothing(ctx, guards):
    from ssdseglib._hip import SsdsegError
    a = 150001
    rng = np.random.default_rng(3)
    corners = guards.inp(AC._grid_corners(a)[None])
    probs = guards.inp(AC.softmax32(rng.normal(0, 1, (1, a, 2))))
    out, valid = guards.out((1, 8, 6)), guards.out(1, np.int32)
    call = lambda a_, sigma, o=out: ctx.call("ssdseg_combined_nms_soft", corners, probs, 1, a_, 2, 4, 8, 0.5, 0.3, sigma, o, valid)
    for sigma in (0.0, -0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(SsdsegError, match=EINVAL(11)):
            call(5, sigma)
    with pytest.raises(SsdsegError, match=EINVAL(5)):
        call(a, 0.5)
    with pytest.raises(SsdsegError, match=EINVAL(5)):                 # the hard entry refuses the same shape
        ctx.call("ssdseg_combined_nms", corners, probs, 1, a, 2, 4, 8, 0.5, 0.3, out, valid)
    with pytest.raises(SsdsegError, match=EINVAL(12)):
        call(5, 0.5, None)
    ctx.sync()
    assert len(guards.unwritten(out)) == 8 * 6 and len(guards.unwritten(valid)) == 1, "a refused call wrote its outputs"
    call(a - 1, 0.5)                                                   # the bound itself is admitted
    assert len(guards.unwritten(out)) == 0 and valid.download()[0] == 8


# ----------------------------------------------------------------------------------------------------------- end to end
def test_predict_and_evaluate_on_device_end_to_end(ctx, guards, trained):
    from ssdseglib import _engine as E, evaluators
    from ssdseglib.layers import soft_nms_reference
    E.set_default_context(ctx)
    sigma = 0.5
    soft_model = trained["builder"].get_model_for_inference(
        model_trained=trained["model"], boxes_iou_threshold=B_THRESHOLD, labels_probability_threshold=P_THRESHOLD,
        use_segmentation_suppression=True, soft_nms_sigma=sigma, **NMS)
    x = trained["images"].astype(np.float32)
    got, want = [], []
    for chunk in (x[:2], x[2:]):
        _, det = soft_model.predict([chunk])
        op = next(op for op in E.engine_for(soft_model, len(chunk), False).ops if isinstance(op, E.DecodeNmsOp))
        assert op.mask is not None and op.nms.soft_nms_sigma == sigma
        corners, probs = op.corners.download(), op.probs_s.download()      # what the op's NMS call read
        ref, _ = soft_nms_reference(corners, probs, NMS["max_number_of_boxes_per_class"], NMS["max_number_of_boxes_per_sample"],
                                    B_THRESHOLD, P_THRESHOLD, sigma)
        got.append(det)
        want.append(ref)
    soft_det, want = np.concatenate(got), np.concatenate(want)
    assert soft_det.shape == (3, NMS["max_number_of_boxes_per_sample"], 6)
    assert np.array_equal(soft_det, want), f"{int((soft_det != want).any(-1).sum())} rows of predict differ from the specification"

    hard_model = inference_model(trained, True)
    assert hard_model.outputs[1].layer.soft_nms_sigma == 0.0
    _, hard_det = predict_batches(hard_model, trained)
    pair, triple = (B_THRESHOLD, P_THRESHOLD), (B_THRESHOLD, P_THRESHOLD, sigma)
    result = evaluators.evaluate_on_device(hard_model, compact_batches(trained), LABELS_CODES, BACKGROUND, [0.5], nms_grid=[pair, triple])
    assert list(result["detections"]) == [pair, triple] and list(result["ap"]) == [pair, triple]
    assert np.array_equal(result["detections"][pair].view(np.uint32), hard_det.view(np.uint32)), "a pair no longer runs the model's own (hard) NMS"
    assert np.array_equal(result["detections"][triple].view(np.uint32), soft_det.view(np.uint32)), "a triple's sigma did not reach the NMS"
    differ = int((soft_det != hard_det).any(-1).sum())
    print(f"detection rows that differ between hard and soft NMS: {differ} of {soft_det.shape[0] * soft_det.shape[1]}")
    assert differ > 0, "hard and soft detections are the same: the test shows nothing"
    # the soft model evaluated with a pair runs its own sigma; a triple with sigma 0 switches it off
    again = evaluators.evaluate_on_device(soft_model, compact_batches(trained), LABELS_CODES, BACKGROUND, [0.5], nms_grid=[pair, pair + (0.0,)])
    assert np.array_equal(again["detections"][pair].view(np.uint32), soft_det.view(np.uint32))
    assert np.array_equal(again["detections"][pair + (0.0,)].view(np.uint32), hard_det.view(np.uint32))
