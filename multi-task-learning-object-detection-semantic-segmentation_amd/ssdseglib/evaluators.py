"""Offline evaluation of saved predictions against ground-truth files (reference evaluators.py:6-247).

Host-side NumPy / CSV / PNG post-processing in the reference too.  Same function names, arguments and return values:
  * `average_precision_object_detection`: per class, predictions of all samples ranked by confidence; a prediction is a true
    positive when its best IoU with a ground-truth box OF THE SAME LABEL reaches the threshold (several predictions may hit the
    same ground-truth box -- the reference does not mark boxes as used); AP = trapezoid area under precision over recall;
  * `jaccard_iou_semantic_segmentation`: the soft Jaccard of the predicted probabilities against one-hot PNG masks, averaged
    over the samples, background dropped from the result.
IoU conventions as everywhere in the reference: pixel-inclusive extents (+1), 1e-7 in the denominator.

`evaluate_on_device` is both of them for a test set the device already holds (compact or resident batches), over a grid of NMS
thresholds (NB03#cell21-29): the masks' Jaccard and the predictions' best IoU are reduced on the GPU (csrc/evaluate.hip), only
the detection rows and a few numbers per image come back, and the ranking tail above runs on them as it does on files.
"""
import csv
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

_EPS = 1e-7


def _iou_boxes_pred_vs_true(labels_pred, boxes_pred, labels_true, boxes_true) -> np.ndarray:
    """(P, T) IoU of predicted vs ground-truth corner boxes, zeroed where the labels differ (reference :6-62); (P, 1) zeros when
    there is no ground truth"""
    boxes_pred = np.asarray(boxes_pred, np.float32).reshape(-1, 4)
    labels_pred = np.asarray(labels_pred).reshape(-1)
    labels_true = np.asarray(labels_true).reshape(-1)
    if labels_true.size == 0:
        return np.zeros((boxes_pred.shape[0], 1), np.float32)
    boxes_true = np.asarray(boxes_true, np.float32).reshape(-1, 4)
    p, t = boxes_pred[:, None, :], boxes_true[None, :, :]
    iw = np.maximum(0.0, np.minimum(p[..., 2], t[..., 2]) - np.maximum(p[..., 0], t[..., 0]) + 1.0)
    ih = np.maximum(0.0, np.minimum(p[..., 3], t[..., 3]) - np.maximum(p[..., 1], t[..., 1]) + 1.0)
    inter = iw * ih
    area_p = (p[..., 2] - p[..., 0] + 1.0) * (p[..., 3] - p[..., 1] + 1.0)
    area_t = (t[..., 2] - t[..., 0] + 1.0) * (t[..., 3] - t[..., 1] + 1.0)
    iou = inter / (area_p + area_t - inter + np.float32(_EPS))
    return (iou * (labels_pred[:, None] == labels_true[None, :])).astype(np.float32)


def _read_labels_boxes(path: str):
    labels, boxes = [], []
    with open(path, "r", newline="") as f:
        for row in csv.reader(f):
            if not row:
                continue
            labels.append(int(row[0]))
            boxes.append([float(v) for v in row[1:5]])
    return np.asarray(labels, np.int32), np.asarray(boxes, np.float32).reshape(-1, 4)


def average_precision_object_detection(labels_pred_batch, confidences_pred_batch, boxes_pred_batch, iou_threshold: float,
                                       path_files_labels_boxes: List[str], labels_codes: List[int], label_code_background: int) -> Dict[int, float]:
    """reference evaluators.py:65-186"""
    classes = [l for l in labels_codes if l != label_code_background]
    hits = {l: [] for l in classes}       # per class: (is true positive, confidence) of every prediction of that class
    n_true = {l: 0 for l in classes}
    for path, lab, conf, box in zip(path_files_labels_boxes, labels_pred_batch, confidences_pred_batch, boxes_pred_batch):
        lt, bt = _read_labels_boxes(path)
        for l in lt:
            n_true[int(l)] += 1
        lab = np.asarray(lab).reshape(-1)
        conf = np.asarray(conf, np.float32).reshape(-1)
        box = np.asarray(box, np.float32).reshape(-1, 4)
        keep = lab != label_code_background
        lab, conf, box = lab[keep], conf[keep], box[keep]
        if lab.size == 0:
            continue
        best = _iou_boxes_pred_vs_true(lab, box, lt, bt).max(axis=1)
        for l, c, tp in zip(lab, conf, best >= iou_threshold):
            hits[int(l)].append((float(tp), float(c)))
    return _average_precision_from_hits(hits, n_true, classes)


def _average_precision_from_hits(hits, n_true, classes) -> Dict[int, float]:
    """the ranking and trapezoid tail of reference evaluators.py:65-186, shared by the host and the device path.  hits: per class the
    (is true positive, confidence) pairs of every prediction of that class, in sample order; n_true: per class the number of
    ground-truth boxes"""
    out = {}
    for l in classes:
        if n_true[l] == 0 or not hits[l]:
            out[l] = 0.0
            continue
        h = np.asarray(hits[l], np.float32)
        order = np.argsort(h[:, 1])[::-1]                 # descending confidence, the reference's tie order
        tp = np.cumsum(h[order, 0])
        precision = tp / np.arange(1, tp.size + 1)
        recall = tp / n_true[l]
        out[l] = float(np.sum((recall[1:] - recall[:-1]) * (precision[1:] + precision[:-1]) * 0.5))   # np.trapz(y=precision, x=recall)
    return out


def jaccard_iou_semantic_segmentation(masks_pred_batch, path_files_masks: List[str], labels_codes: List[int],
                                      label_code_background: int) -> Dict[int, float]:
    """reference evaluators.py:189-247"""
    from PIL import Image
    pred = np.asarray(masks_pred_batch, np.float32)
    n_cls = len(labels_codes)
    classes = np.arange(n_cls)
    # one-hot of the single-channel PNG (pixel value = class label; values >= n_cls give an all-zero pixel, as tf.one_hot does)
    true = np.stack([(np.asarray(Image.open(p).convert("L"), np.int64)[..., None] == classes).astype(np.float32) for p in path_files_masks])
    inter = (true * pred).sum(axis=(1, 2))
    total = (true + pred).sum(axis=(1, 2))
    iou = (inter / (total - inter + np.float32(_EPS))).mean(axis=0)
    return {l: float(v) for l, v in zip(labels_codes, iou) if l != label_code_background}


def confusion_matrix_semantic_segmentation(masks_pred_batch, masks_true_index, n_classes: int) -> Tuple[np.ndarray, int]:
    """The hard confusion matrix of saved predictions (not in the reference), and the spec of the device path
    (ssdseg_eval_mask_scores).  masks_pred_batch: (N, H, W, C) probabilities; masks_true_index: (N, H, W) class indices (an
    index >= n_classes is void).  For every labelled pixel of class k: M[k][argmax_c p_c] += 1, the lowest index among equal
    probabilities (np.argmax); void pixels enter no row.  -> (M (C, C) int64, rows true and columns predicted; void pixels)"""
    n_classes = int(n_classes)
    pred = np.asarray(masks_pred_batch)
    true = np.asarray(masks_true_index).astype(np.int64)
    if pred.shape[-1] != n_classes or pred.shape[:-1] != true.shape:
        raise ValueError(f"predictions {pred.shape} do not fit class indices {true.shape} with {n_classes} classes")
    labelled = (true >= 0) & (true < n_classes)
    cells = true[labelled] * n_classes + pred.argmax(axis=-1)[labelled]
    m = np.bincount(cells, minlength=n_classes * n_classes).reshape(n_classes, n_classes).astype(np.int64)
    return m, int(true.size - labelled.sum())


def scores_from_confusion(confusion, labels_codes: List[int]) -> Tuple[Dict[int, float], float, float]:
    """-> (iou_hard {label: M_cc / (row_c + col_c - M_cc), NaN for a class neither labelled nor predicted}, miou: its mean over
    the classes that are not NaN, background included (the VOC / Cityscapes convention; NaN when every class is),
    pixel_accuracy: trace / sum (NaN for an empty matrix))"""
    m = np.asarray(confusion, np.int64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] != len(labels_codes):
        raise ValueError(f"confusion matrix {m.shape} for {len(labels_codes)} label codes")
    diag = np.diag(m).astype(np.float64)
    den = (m.sum(axis=1) + m.sum(axis=0)).astype(np.float64) - diag
    iou = np.full(m.shape[0], np.nan)
    np.divide(diag, den, out=iou, where=den > 0)
    seen = ~np.isnan(iou)
    miou = float(iou[seen].mean()) if seen.any() else float("nan")
    total = int(m.sum())
    return {l: float(v) for l, v in zip(labels_codes, iou)}, miou, (float(np.trace(m)) / total if total else float("nan"))


def _nms_layer(model_inference):
    for t in model_inference.outputs:
        if type(t.layer).__name__ == "NonMaximumSuppression":
            return t.layer
    raise ValueError("evaluate_on_device needs a model from get_model_for_inference (no NMS output in this one)")


def _grid_entry(entry) -> tuple:
    """one nms_grid entry as a tuple of floats: (b_thr, p_thr), or (b_thr, p_thr, sigma) with a Soft-NMS sigma >= 0"""
    from .layers import soft_nms_sigma_value
    entry = tuple(entry)
    if len(entry) not in (2, 3):
        raise ValueError(f"evaluate_on_device: an nms_grid entry is (boxes_iou_threshold, labels_probability_threshold) or "
                         f"(boxes_iou_threshold, labels_probability_threshold, soft_nms_sigma), got {entry!r}")
    return (float(entry[0]), float(entry[1])) + tuple(soft_nms_sigma_value(s) for s in entry[2:])


_NOT_PLAIN = {"rgb_draws": "the batch carries colour-augmentation draws",
              "crop_windows": "the batch carries crop windows; a test set is not augmented",
              "mosaic": "the batch carries a mosaic; a test set is not augmented",
              "flip": "the batch has mirrored samples (flip flags set)"}


def _check_plain(batch) -> None:
    """evaluation is on the files as they are: no mirrored sample, no colour draws, no crop windows, no mosaic"""
    kind = type(batch).__name__
    if kind not in ("CompactBatch", "ResidentBatch"):
        raise ValueError(f"evaluate_on_device takes CompactBatch / ResidentBatch objects or a ResidentDataset, got {kind}")
    for carried in batch.augmented_by():
        raise ValueError("evaluate_on_device: " + _NOT_PLAIN[carried])


def _plain_batches(data):
    if type(data).__name__ == "ResidentDataset":
        # slot order in the dataset's batch size, whatever its shuffle / flip / colour settings; its generator is not consumed
        n, b = data.num_samples, data.batch_size
        cuts = [(lo, min(lo + b, n)) for lo in range(0, n, b)]
        data = [data.batch(np.arange(lo, hi, dtype=np.int32)) for lo, hi in cuts if not (data.drop_remainder and hi - lo < b)]
    elif isinstance(data, (list, tuple)):
        for batch in data:                      # a list is checked as a whole before the first batch reaches the device
            _check_plain(batch)
    for batch in data:
        _check_plain(batch)
        yield batch


def _labels_true(batch) -> List[np.ndarray]:
    """per sample the labels of its ground-truth rows, from the host's copy"""
    if type(batch).__name__ == "ResidentBatch":
        return [batch.dataset._gt_labels[int(i)] for i in batch.index]
    return [g[:, 0].astype(np.int32) for g in batch.ground_truth]


def evaluate_on_device(model_inference, data, labels_codes: List[int], label_code_background: int, iou_thresholds: Sequence[float],
                       nms_grid: Optional[Iterable[Tuple[float, ...]]] = None, ignore_void: bool = False, confusion: bool = False) -> dict:
    """The test-set evaluation of NB03#cell21-29 on a set the device holds.

    model_inference: from `get_model_for_inference` (suppress_background_boxes=False: with True the detections lose their batch
    axis, quirk Q7, and belong to no image; use_segmentation_suppression either way).  data: an iterable of
    `datacoder.CompactBatch`, a `ResidentDataset` (walked in slot order in its batch size, un-augmented, its generator untouched)
    or an iterable of `ResidentBatch`; no flips, no colour draws, no crop windows (ValueError).  nms_grid: (boxes_iou_threshold, labels_probability_threshold)
    pairs or (boxes_iou_threshold, labels_probability_threshold, soft_nms_sigma) triples, default the model's own thresholds.  A
    pair runs with the model's own soft_nms_sigma; a triple's sigma of 0 is the hard NMS, above 0 Gaussian Soft-NMS
    (layers.soft_nms_reference; a negative or non-finite sigma or an entry of another length: ValueError).  Per batch the network
    and the decode (+ segmentation suppression) run once, the NMS once per entry: a sigma sweep costs no network pass.
    Segmentation suppression is batch-wide (quirk Q6), so the detections are those of `predict` on the same batches.

    -> {'iou': {label: soft Jaccard, mean over the samples (float64, sample order)},
        'ap': {entry: {iou_threshold: {label: average precision}}},
        'detections': {entry: (N, r, 6) rows (label, confidence, xmin, ymin, xmax, ymax)}}
    with entry = the nms_grid entry as passed, as a tuple of floats: (b_thr, p_thr) or (b_thr, p_thr, sigma);
    without the background in 'iou' and 'ap', as jaccard_iou_semantic_segmentation / average_precision_object_detection, whose
    values these are (rows of label 0 are empty NMS rows and never count as predictions).

    ignore_void=True: 'iou' sums total = sum (y + p) over the labelled pixels only; a void pixel (class index >= the number of
    classes) then enters neither sum.  confusion=True adds the hard scores every segmentation paper reports, from arg-max
    predictions accumulated over the whole set with void excluded (whatever ignore_void says):
        'confusion': (C, C) int64, rows true, columns predicted;  'void_pixels': int;
        'iou_hard': {label: IoU} for EVERY label code, background included (NaN for an absent class);
        'miou': their mean without the NaNs;  'pixel_accuracy': trace / sum
    (confusion_matrix_semantic_segmentation / scores_from_confusion on `predict`'s masks).  Either option sends the batch through
    ssdseg_eval_mask_scores: the probabilities are still read once."""
    from .losses import void_flag
    ignore_void = void_flag(ignore_void)
    if not isinstance(confusion, (bool, np.bool_)):
        raise ValueError(f"confusion must be a bool, got {confusion!r}")
    nms = _nms_layer(model_inference)
    if nms.suppress_background_boxes:
        raise ValueError("evaluate_on_device: suppress_background_boxes=True drops the batch axis of the detections (quirk Q7)")
    labels_codes = list(labels_codes)
    n_cls = int(model_inference.outputs[0].shape[-1])
    if len(labels_codes) != n_cls:
        raise ValueError(f"{len(labels_codes)} label codes for a mask output of {n_cls} classes")
    pairs = [(float(nms.boxes_iou_threshold), float(nms.labels_probability_threshold))] if nms_grid is None \
        else [_grid_entry(entry) for entry in nms_grid]
    thresholds = [float(t) for t in iou_thresholds]
    if not pairs or not thresholds:
        raise ValueError("evaluate_on_device: empty nms_grid or iou_thresholds")
    classes = [l for l in labels_codes if l != label_code_background]
    hits = {pair: {t: {l: [] for l in classes} for t in thresholds} for pair in pairs}
    n_true = {l: 0 for l in classes}
    detections = {pair: [] for pair in pairs}
    iou_sum, seen = np.zeros(n_cls, np.float64), 0
    matrix, void_pixels = np.zeros((n_cls, n_cls), np.int64), 0

    from . import _fit
    for batch in _plain_batches(data):
        if ignore_void or confusion:
            iou, per_pair, counts = _fit.run_evaluate_scores(model_inference, batch, pairs, ignore_void, bool(confusion))
            if counts is not None:
                matrix += counts[0].astype(np.int64).sum(axis=0)
                void_pixels += int(counts[1].astype(np.int64).sum())
        else:
            iou, per_pair = _fit.run_evaluate(model_inference, batch, pairs)
        for row in iou:
            iou_sum += row.astype(np.float64)
            seen += 1
        for lt in _labels_true(batch):
            for l in lt:
                n_true[int(l)] += 1
        for pair, (det, best) in per_pair.items():
            detections[pair].append(det)
            for d, b in zip(det, best):
                lab = d[:, 0].astype(np.int32)
                keep = (lab != label_code_background) & (lab != 0)
                for t in thresholds:
                    for l, c, tp in zip(lab[keep], d[keep, 1], b[keep] >= t):
                        hits[pair][t][int(l)].append((float(tp), float(c)))
    if seen == 0:
        raise ValueError("evaluate_on_device: no samples")
    mean = iou_sum / seen
    result = {"iou": {l: float(v) for l, v in zip(labels_codes, mean) if l != label_code_background},
              "ap": {pair: {t: _average_precision_from_hits(hits[pair][t], n_true, classes) for t in thresholds} for pair in pairs},
              "detections": {pair: np.concatenate(detections[pair], axis=0) for pair in pairs}}
    if confusion:
        iou_hard, miou, accuracy = scores_from_confusion(matrix, labels_codes)
        result.update(confusion=matrix, void_pixels=void_pixels, iou_hard=iou_hard, miou=miou, pixel_accuracy=accuracy)
    return result
