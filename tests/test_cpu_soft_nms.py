"""Soft-NMS (Gaussian score decay) without a GPU: the NumPy specification `layers.soft_nms_reference` and the Python surface.

1. A sigma so large that every weight rounds to 1 (1e30) is the hard NMS: the specification equals oracle.np_ops.combined_nms
   `array_equal` on every case of tests/_anchor_cases.py but the 150000-anchor one (tests/test_gpu_soft_nms.py runs that one).
2. A hand-worked case on the boxes of `nms_exact_iou_threshold`, every property asserted on the specification alone: a pair with
   IoU exactly 0.5 decays at iou_thr = 0.5 (the comparison is strict) and dies one float32 below it; a candidate whose decayed
   score lands under the score threshold dies softly; a pair changes places in the merged output because of the decay.  The `dry`
   case loses one detection per image the same way.
3. The surface: the layer's argument check and config, evaluate_on_device's grid entries (rejected before any device is
   touched), the new symbol in the header with the ctypes signature.
"""
import os
import re

import numpy as np
import pytest

import _anchor_cases as AC

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CASES = [name for name in AC.NMS_CASES if name != "bound-150000"]


def soft(inputs, corners, sigma, **override):
    from ssdseglib.layers import soft_nms_reference
    k = {**inputs, **override}
    return soft_nms_reference(corners, k["probs"], k["max_per_class"], k["max_total"], k["iou_thr"], k["score_thr"], sigma)


def weight(iou, sigma):
    """the specification's weight, written out once more: float32(exp(-0.5 * x * x / float64(float32(sigma))))"""
    x = np.float64(F32(iou))
    return F32(np.exp(-0.5 * x * x / np.float64(F32(sigma))))


# --------------------------------------------------------------------------------------------- 1. large sigma == the hard NMS
@pytest.mark.parametrize("name", SMALL_CASES)
def test_large_sigma_is_the_hard_nms(name):
    inputs, _ = AC.NMS_CASES[name]()
    corners = AC.oracle_corners(inputs)
    want, want_valid = AC.oracle_nms(inputs, corners)
    got, got_valid = soft(inputs, corners, 1e30)
    assert got.dtype == np.float32 and got_valid.dtype == np.int32
    assert np.array_equal(got_valid, want_valid)
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} rows differ"


def test_weight_is_one_at_zero_overlap_and_at_a_huge_sigma():
    assert weight(0.0, 0.5) == F32(1) and weight(1.0, 1e30) == F32(1) and weight(0.999, 1e30) == F32(1)
    assert weight(0.5, 0.5) == F32(np.exp(-0.25)) and F32(0.7788) < weight(0.5, 0.5) < F32(0.7789)


# --------------------------------------------------------------------------------------------------------- 2. hand-worked
def rows_of(out, valid, image=0):
    """[(label, score, anchor-identifying xmin, ymin, xmax, ymax)] of the real rows"""
    return [tuple(float(v) for v in r) for r in out[image, :valid[image]]]


def test_hand_worked_decay_on_the_threshold():
    """anchors 0 .. 4 = (0,0,1,2) 0.9, (0,0,1,1) 0.8, (10,10,12,12) 0.7, (20,20,21,24) 0.5, (20,20,21,22) 0.75 in class 1, score
    threshold 0.45; anchors (0, 1) and (3, 4) have IoU exactly 0.5, everything else is disjoint.  Class 0 holds 1 - these: only
    anchor 3 (0.5) is above the threshold there."""
    inputs, _ = AC.nms_exact_iou_threshold(0.5)
    corners, probs = inputs["corners"], inputs["probs"]
    w = weight(0.5, 0.5)
    assert w == F32(np.exp(-0.25))
    s = probs[0, :, 1]

    out, valid = soft(inputs, corners, 0.5)
    # class 1: 0 (0.9); 1 decays to 0.8 w = 0.623; 4 (0.75) is picked next and decays 3 to 0.5 w = 0.389 <= 0.45: a soft death
    # (its IoU of 0.5 is not above the threshold); then 2 (0.7), then 1 with its decayed score.  Class 0: anchor 3 alone, undecayed.
    decayed_1, decayed_3 = F32(s[1] * w), F32(s[3] * w)
    assert decayed_3 <= F32(inputs["score_thr"]) < s[3], "anchor 3 dies by decay, not by its own score"
    assert F32(inputs["score_thr"]) < decayed_1 < s[2] < s[1], "anchor 1 survives the decay and falls behind anchor 2"
    want = [(1, s[0], 0), (1, s[4], 4), (1, s[2], 2), (1, decayed_1, 1), (0, probs[0, 3, 0], 3)]
    want.sort(key=lambda t: (-float(t[1]), t[2], t[0]))
    assert valid.tolist() == [5]
    for row, (label, score, anchor) in zip(out[0], want):
        y0, x0, y1, x1 = corners[0, anchor]
        assert np.array_equal(row, np.array([label, score, x0, y0, x1, y1], F32)), (row, label, score, anchor)
    assert not out[0, 5:].any()
    assert np.array_equal(out[0, 3, 1], decayed_1) and out[0, 3, 1] == F32(F32(0.8) * F32(np.exp(-0.25)))

    # the hard NMS on the same inputs keeps all six, anchor 1 (0.8) ahead of anchors 4 (0.75) and 2 (0.7): the decay flips the order
    hard, hard_valid = AC.oracle_nms(inputs, corners)
    assert hard_valid.tolist() == [6]
    xyxy = corners[0][:, [1, 0, 3, 2]]
    order = lambda o, n: [int(np.flatnonzero((xyxy == r[2:]).all(-1))[0]) for r in o[0, :n] if r[0] == 1]      # class 1's anchors, row order
    assert order(hard, 6) == [0, 1, 4, 2, 3] and order(out, 5) == [0, 4, 2, 1]

    # one float32 below 0.5 both partners die by the hard step, whatever sigma says
    below, below_valid = soft(inputs, corners, 0.5, iou_thr=AC.HALF_BELOW)
    hard_below, hard_below_valid = AC.oracle_nms(inputs, corners, iou_thr=AC.HALF_BELOW)
    assert below_valid.tolist() == hard_below_valid.tolist() == [4]
    assert np.array_equal(below, hard_below), "nothing but disjoint boxes left: every weight is 1"
    assert order(below, 4) == [0, 4, 2]

    # iou_thr = 1: no hard step at all; at a small sigma the overlapping partners decay under the score threshold
    pure, pure_valid = soft(inputs, corners, 0.1, iou_thr=1.0)
    assert F32(s[1] * weight(0.5, 0.1)) <= F32(inputs["score_thr"])
    assert pure_valid.tolist() == [4] and order(pure, 4) == [0, 4, 2]


def test_dry_case_loses_one_detection_per_image_to_the_decay():
    inputs, _ = AC.nms_dry()
    corners = AC.oracle_corners(inputs)
    _, hard_valid = AC.oracle_nms(inputs, corners)
    out, valid = soft(inputs, corners, 0.5)
    assert hard_valid.tolist() == [36, 35] and valid.tolist() == [35, 34]
    hard_all, _ = AC.oracle_nms(inputs, corners)
    for img in range(2):
        assert not out[img, valid[img]:].any()
        for cls in range(inputs["c"]):                                 # a class's scores only shrink: non-increasing, never above the hard ones
            mine = out[img, :valid[img]][out[img, :valid[img], 0] == cls][:, 1]
            theirs = hard_all[img, :hard_valid[img]][hard_all[img, :hard_valid[img], 0] == cls][:, 1]
            assert (np.diff(mine) <= 0).all() and mine.max() <= theirs.max() and (mine > F32(inputs["score_thr"])).all()
    assert (out[..., 1] != hard_all[..., 1]).any()


def test_reference_rejects_a_sigma_that_is_off():
    inputs, _ = AC.nms_exact_iou_threshold(0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "0.5", None):
        with pytest.raises(ValueError, match="soft_nms_sigma"):
            soft(inputs, inputs["corners"], bad)


# ------------------------------------------------------------------------------------------------------------ 3. the surface
LAYER = dict(max_number_of_boxes_per_class=4, max_number_of_boxes_per_sample=10, boxes_iou_threshold=0.3, labels_probability_threshold=0.4,
             suppress_background_boxes=False)


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), -float("inf"), "0.5", None, [0.5], True, 1e-60, 1e60])
def test_layer_rejects_a_bad_sigma(bad):
    from ssdseglib import layers
    with pytest.raises(ValueError, match="soft_nms_sigma"):
        layers.NonMaximumSuppression(soft_nms_sigma=bad, **LAYER)


def test_layer_config_round_trip():
    from ssdseglib import layers
    assert layers.NonMaximumSuppression(**LAYER).soft_nms_sigma == 0.0
    assert layers.NonMaximumSuppression(**LAYER).get_config() == {**LAYER, "soft_nms_sigma": 0.0}
    layer = layers.NonMaximumSuppression(soft_nms_sigma=np.float32(0.5), name="nms", **LAYER)
    config = layer.get_config()
    assert config == {**LAYER, "soft_nms_sigma": 0.5} and type(config["soft_nms_sigma"]) is float
    again = layers.NonMaximumSuppression(**config)
    assert again.get_config() == config
    assert layers.NonMaximumSuppression(soft_nms_sigma=1, **LAYER).soft_nms_sigma == 1.0


def test_inference_model_carries_sigma():
    from tests.test_cpu_evaluate import _small_inference_model
    nms = lambda m: next(t.layer for t in m.outputs if type(t.layer).__name__ == "NonMaximumSuppression")
    assert nms(_small_inference_model()).soft_nms_sigma == 0.0
    assert nms(_small_inference_model(soft_nms_sigma=0.25)).soft_nms_sigma == 0.25
    with pytest.raises(ValueError, match="soft_nms_sigma"):
        _small_inference_model(soft_nms_sigma=-1.0)


@pytest.mark.parametrize("grid,what", [([(0.3, 0.4, 0.5, 0.1)], "nms_grid entry"), ([(0.3, 0.4), (0.3,)], "nms_grid entry"),
                                       ([(0.3, 0.4, -0.5)], "soft_nms_sigma"), ([(0.3, 0.4), (0.3, 0.4, float("nan"))], "soft_nms_sigma"),
                                       ([(0.3, 0.4, "wide")], "soft_nms_sigma")])
def test_evaluate_on_device_rejects_bad_grid_entries(monkeypatch, grid, what):
    from tests.test_cpu_evaluate import BACKGROUND, LABELS_CODES, _compact, _small_inference_model
    from ssdseglib import _engine, _fit, _hip, evaluators

    def refuse(*a, **k):
        raise AssertionError("evaluate_on_device touched the device before rejecting its arguments")

    monkeypatch.setattr(_hip.Context, "__init__", refuse)
    monkeypatch.setattr(_engine, "engine_for", refuse)
    monkeypatch.setattr(_fit, "run_evaluate", refuse)
    with pytest.raises(ValueError, match=what):
        evaluators.evaluate_on_device(_small_inference_model(), [_compact()], LABELS_CODES, BACKGROUND, [0.5], nms_grid=grid)


def test_evaluate_on_device_keys_are_the_entries_as_floats(monkeypatch):
    """a pair reaches the engine as a pair (the model's own sigma), a triple as a triple; the result is keyed by them"""
    from tests.test_cpu_evaluate import BACKGROUND, LABELS_CODES, _compact, _small_inference_model
    from ssdseglib import _fit, evaluators
    seen = []

    def fake(model, batch, pairs):
        seen.append(list(pairs))
        return np.zeros((2, 4), np.float32), {p: (np.zeros((2, 10, 6), np.float32), np.zeros((2, 10), np.float32)) for p in pairs}

    monkeypatch.setattr(_fit, "run_evaluate", fake)
    grid = [(0.3, 0.4), [np.float32(0.5), 0.25, 1], (0.3, 0.4, 0.0)]
    result = evaluators.evaluate_on_device(_small_inference_model(), [_compact()], LABELS_CODES, BACKGROUND, [0.5], nms_grid=grid)
    keys = [(0.3, 0.4), (0.5, 0.25, 1.0), (0.3, 0.4, 0.0)]
    assert seen == [keys] and list(result["detections"]) == keys and list(result["ap"]) == keys
    assert all(type(v) is float for key in result["detections"] for v in key)


def test_symbol_in_the_header_with_its_signature():
    import ctypes as C
    from ssdseglib import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ssdseg.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ssdseg_combined_nms_soft\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m, "ssdseg_combined_nms_soft is not declared in include/ssdseg.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["ssdseg_ctx* ctx", "const float* corners", "const float* probs", "int b", "int a", "int c", "int max_per_class",
                      "int max_total", "float iou_threshold", "float score_threshold", "float soft_nms_sigma", "float* out", "int32_t* valid"]
    want = [C.c_float if p.startswith("float ") else C.c_int if p.startswith("int ") else C.c_void_p for p in params]
    assert _hip._SIGNATURES["ssdseg_combined_nms_soft"] == want
    assert _hip._SIGNATURES["ssdseg_combined_nms_soft"] == _hip._SIGNATURES["ssdseg_combined_nms"][:10] + [C.c_float] + \
        _hip._SIGNATURES["ssdseg_combined_nms"][10:]
    assert "ssdseg_combined_nms_soft" in _hip.declared_symbols()
