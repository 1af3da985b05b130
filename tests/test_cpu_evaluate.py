"""Host side of `evaluators.evaluate_on_device`, without a GPU: the average-precision tail that the host and the device path now
share still gives what `average_precision_object_detection` gave before it was factored out (the expected values below are the
output of the function as it stood before, on this very case), the argument checks fire before any device is touched, and the two
new C-ABI entry points are declared, bound and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LABELS_CODES, BACKGROUND = [0, 1, 2, 3], 0

# 3 images; class 3 has predictions but no ground truth; image 1 has no predictions; confidences all distinct
GROUND_TRUTH = [
    [(1, 10, 10, 50, 50), (2, 60, 20, 100, 70)],
    [(1, 5, 5, 40, 45)],
    [(2, 20, 20, 60, 60), (1, 70, 70, 110, 100)],
]
# (label, confidence, xmin, ymin, xmax, ymax)
PREDICTIONS = [
    [(1, 0.90, 12, 11, 49, 52), (2, 0.80, 0, 0, 20, 20), (1, 0.35, 10, 10, 50, 50), (3, 0.60, 60, 20, 100, 70), (0, 0.99, 10, 10, 50, 50),
     (2, 0.20, 58, 22, 97, 71)],
    [],
    [(2, 0.70, 22, 18, 61, 63), (1, 0.55, 75, 72, 108, 99), (1, 0.45, 0, 0, 30, 30), (2, 0.30, 90, 90, 120, 120), (1, 0.95, 0, 50, 40, 90)],
]
# average_precision_object_detection on the case above as it was before the tail moved into _average_precision_from_hits
EXPECTED = {
    0.5: {1: 0.46111110846201575, 2: 0.3333333333333333, 3: 0.0},
    0.75: {1: 0.19166667237877846, 2: 0.3333333333333333, 3: 0.0},
}


def _pred_arrays():
    labels, confidences, boxes = [], [], []
    for rows in PREDICTIONS:
        a = np.asarray(rows, np.float32).reshape(-1, 6)
        labels.append(a[:, 0].astype(np.int32))
        confidences.append(a[:, 1])
        boxes.append(a[:, 2:])
    return labels, confidences, boxes


def _write_csvs(tmp_path):
    paths = []
    for i, rows in enumerate(GROUND_TRUTH):
        p = tmp_path / f"sample{i}.csv"
        p.write_text("".join(",".join(str(v) for v in r) + "\n" for r in rows))
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("threshold", sorted(EXPECTED))
def test_average_precision_is_what_it_was(tmp_path, threshold):
    from ssdseglib import evaluators
    labels, confidences, boxes = _pred_arrays()
    got = evaluators.average_precision_object_detection(labels, confidences, boxes, threshold, _write_csvs(tmp_path), LABELS_CODES, BACKGROUND)
    assert got == EXPECTED[threshold], got


@pytest.mark.parametrize("threshold", sorted(EXPECTED))
def test_shared_tail_from_hits(threshold):
    """the helper fed the (true positive, confidence) pairs directly -- the best IoUs computed here per image, thresholded as the
    device path thresholds the kernel's output"""
    from ssdseglib import evaluators
    classes = [1, 2, 3]
    hits = {l: [] for l in classes}
    n_true = {l: 0 for l in classes}
    labels, confidences, boxes = _pred_arrays()
    for gt, lab, conf, box in zip(GROUND_TRUTH, labels, confidences, boxes):
        gt = np.asarray(gt, np.float32).reshape(-1, 5)
        for l in gt[:, 0]:
            n_true[int(l)] += 1
        if lab.size == 0:
            continue
        best = evaluators._iou_boxes_pred_vs_true(lab, box, gt[:, 0].astype(np.int32), gt[:, 1:]).max(axis=1)
        for l, c, b in zip(lab, conf, best):
            if l != BACKGROUND:
                hits[int(l)].append((float(b >= threshold), float(c)))
    assert n_true == {1: 3, 2: 2, 3: 0}
    assert evaluators._average_precision_from_hits(hits, n_true, classes) == EXPECTED[threshold]


# ------------------------------------------------------------------------------------------------ argument checks, no device
def _small_inference_model(**kw):
    import ssdseglib
    from ssdseglib import _graph as K
    K.set_seed(5)
    shape, fmaps, stds = (96, 128, 3), ((6, 8), (3, 4), (2, 2), (1, 1)), (0.1, 0.1, 0.2, 0.2)
    boxes = ssdseglib.boxes.DefaultBoundingBoxes(feature_maps_shapes=fmaps, centers_padding_from_borders_percentage=0.05, boxes_scales=(0.15, 0.95))
    boxes.rescale_boxes_coordinates(shape[:2])
    builder = ssdseglib.models.MobileNetV2SsdSegBuilder(
        shape, [6, 6, 6, 6], 4, boxes.get_boxes_coordinates_center_x('ssd'), boxes.get_boxes_coordinates_center_y('ssd'),
        boxes.get_boxes_coordinates_width('ssd'), boxes.get_boxes_coordinates_height('ssd'), stds)
    model = builder.get_model_for_training('deeplabv3plus', 'ssdlite', (3, 6, 12))
    args = dict(model_trained=model, max_number_of_boxes_per_class=4, max_number_of_boxes_per_sample=10, boxes_iou_threshold=0.3,
                labels_probability_threshold=0.4, suppress_background_boxes=False, use_segmentation_suppression=True)
    args.update(kw)
    return builder.get_model_for_inference(**args)


def _compact(flip=None, rgb_draws=None):
    import ssdseglib
    img = np.zeros((2, 96, 128, 3), np.uint8)
    return ssdseglib.datacoder.CompactBatch(img, np.zeros((2, 96, 128), np.uint8), [np.zeros((0, 5), np.float32)] * 2, flip, None, rgb_draws=rgb_draws)


@pytest.fixture()
def no_device(monkeypatch):
    """any attempt to open a device context or to lower an engine fails the test"""
    from ssdseglib import _engine, _fit, _hip

    def refuse(*a, **k):
        raise AssertionError("evaluate_on_device touched the device before rejecting its arguments")

    monkeypatch.setattr(_hip.Context, "__init__", refuse)
    monkeypatch.setattr(_engine, "engine_for", refuse)
    monkeypatch.setattr(_fit, "run_evaluate", refuse)


def test_rejects_suppress_background_boxes(no_device):
    from ssdseglib import evaluators
    model = _small_inference_model(suppress_background_boxes=True)
    with pytest.raises(ValueError, match="suppress_background_boxes"):
        evaluators.evaluate_on_device(model, [_compact()], LABELS_CODES, BACKGROUND, [0.5])


@pytest.mark.parametrize("kind", ["flip", "draws", "flip in the second batch of a list", "flip from a generator"])
def test_rejects_augmented_batches(no_device, kind):
    from ssdseglib import evaluators
    model = _small_inference_model()
    if kind == "flip":
        data = [_compact(flip=[0, 1])]
    elif kind == "draws":
        data = [_compact(rgb_draws=(0.01, 1.0, 1.0, 0.0))]
    elif kind == "flip in the second batch of a list":
        data = [_compact(flip=[0, 0]), _compact(flip=[1, 0])]
    else:
        data = (b for b in [_compact(flip=[0, 1])])
    with pytest.raises(ValueError, match="mirrored|colour"):
        evaluators.evaluate_on_device(model, data, LABELS_CODES, BACKGROUND, [0.5])


def test_rejects_other_argument_errors(no_device):
    from ssdseglib import evaluators
    model = _small_inference_model()
    with pytest.raises(ValueError, match="label codes"):
        evaluators.evaluate_on_device(model, [_compact()], [0, 1, 2], BACKGROUND, [0.5])
    with pytest.raises(ValueError, match="empty"):
        evaluators.evaluate_on_device(model, [_compact()], LABELS_CODES, BACKGROUND, [])
    with pytest.raises(ValueError, match="CompactBatch"):
        evaluators.evaluate_on_device(model, [np.zeros((2, 96, 128, 3), np.float32)], LABELS_CODES, BACKGROUND, [0.5])


# ------------------------------------------------------------------------------------------------------------- the C-ABI
NEW_SYMBOLS = {
    "ssdseg_eval_mask_jaccard": ["ssdseg_ctx*", "const float*", "const uint8_t*", "int", "int", "int", "float*"],
    "ssdseg_eval_det_best_iou": ["ssdseg_ctx*", "const float*", "const float*", "const int32_t*", "int", "int", "int", "float*"],
}


def test_new_entry_points_are_declared_bound_and_exported():
    from ssdseglib import _hip
    header = open(os.path.join(REPO, "include", "ssdseg.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _hip.load_library()
    for name, want in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in include/ssdseg.h"
        params = [re.sub(r"\s*\w+$", "", p.strip()) for p in m.group(1).replace("\n", " ").split(",")]
        assert params == want, (name, params)
        sig = _hip._SIGNATURES[name]
        assert len(sig) == len(want)
        for ct, p in zip(sig, want):
            assert ct is (C.c_int if p == "int" else C.c_void_p), (name, p, ct)
        assert name in _hip.declared_symbols() and hasattr(lib, name)
        assert getattr(lib, name).argtypes == sig and getattr(lib, name).restype is C.c_int


def test_new_entry_points_report_bad_arguments_without_a_device():
    """the usual status convention: -1000 - n for bad argument n, checked before anything is launched"""
    from ssdseglib import _hip
    lib = _hip.load_library()
    assert lib.ssdseg_eval_mask_jaccard(None, None, None, 1, 1, 4, None) == -1001
    assert lib.ssdseg_eval_det_best_iou(None, None, None, None, 1, 1, 1, None) == -1001
    assert b"ssdseg_eval_det_best_iou" in lib.ssdseg_last_error()
