"""Custom layers of the inference tail -- same constructor kwargs as the reference (layers.py:6-17, :97-105, :181,
:216).  As graph nodes they are lowered by `_engine.py` to the HIP kernels ssdseg_decode_boxes /
ssdseg_combined_nms (ssdseg_combined_nms_soft with soft_nms_sigma > 0; `soft_nms_reference` is its NumPy specification) /
ssdseg_seg_suppress; `Split` is a zero-copy channel view.
"""
from typing import List, Union

import numpy as np

from . import _graph as K


class DecodeBoxesCentroidsOffsets(K.Layer):
    """Predicted centroid offsets -> corners (ymin, xmin, ymax, xmax) (reference layers.py:45-81)."""
    type_name = "DecodeBoxesCentroidsOffsets"

    def __init__(self, center_x_boxes_default, center_y_boxes_default, width_boxes_default, height_boxes_default,
                 standard_deviation_center_x_offsets: float, standard_deviation_center_y_offsets: float,
                 standard_deviation_width_offsets: float, standard_deviation_height_offsets: float, **kwargs):
        super().__init__(**kwargs)
        self.center_x_boxes_default = np.asarray(center_x_boxes_default, np.float32)
        self.center_y_boxes_default = np.asarray(center_y_boxes_default, np.float32)
        self.width_boxes_default = np.asarray(width_boxes_default, np.float32)
        self.height_boxes_default = np.asarray(height_boxes_default, np.float32)
        self.standard_deviation_center_x_offsets = float(standard_deviation_center_x_offsets)
        self.standard_deviation_center_y_offsets = float(standard_deviation_center_y_offsets)
        self.standard_deviation_width_offsets = float(standard_deviation_width_offsets)
        self.standard_deviation_height_offsets = float(standard_deviation_height_offsets)

    def get_config(self):
        return {k: getattr(self, k) for k in (
            'center_x_boxes_default', 'center_y_boxes_default', 'width_boxes_default', 'height_boxes_default',
            'standard_deviation_center_x_offsets', 'standard_deviation_center_y_offsets',
            'standard_deviation_width_offsets', 'standard_deviation_height_offsets')}


def soft_nms_sigma_value(sigma, allow_zero: bool = True) -> float:
    """a soft_nms_sigma argument as the float the C-ABI receives: a finite number >= 0 (0 is off), ValueError otherwise"""
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)):
        raise ValueError(f"soft_nms_sigma must be a number, got {sigma!r}")
    value = float(sigma)
    if not np.isfinite(value) or value < 0 or (value == 0 and not allow_zero):
        raise ValueError(f"soft_nms_sigma must be finite and {'>=' if allow_zero else '>'} 0, got {sigma!r}")
    with np.errstate(all="ignore"):
        as_f32 = np.float64(value).astype(np.float32)
    if value > 0 and not (np.isfinite(as_f32) and as_f32 > 0):
        raise ValueError(f"soft_nms_sigma {sigma!r} is not a positive finite float32")
    return value


class NonMaximumSuppression(K.Layer):
    """Combined per-class NMS + repack to (label, prob, xmin, ymin, xmax, ymax) (reference layers.py:127-168).
    soft_nms_sigma > 0 (not in the reference): Gaussian Soft-NMS, a box that overlaps a kept one by no more than
    boxes_iou_threshold keeps a decayed score instead of its own (`soft_nms_reference` is the definition); 0.0 is off."""
    type_name = "NonMaximumSuppression"

    def __init__(self, max_number_of_boxes_per_class: int, max_number_of_boxes_per_sample: int, boxes_iou_threshold: float,
                 labels_probability_threshold: float, suppress_background_boxes: bool, soft_nms_sigma: float = 0.0, **kwargs):
        super().__init__(**kwargs)
        self.max_number_of_boxes_per_class = max_number_of_boxes_per_class
        self.max_number_of_boxes_per_sample = max_number_of_boxes_per_sample
        self.boxes_iou_threshold = boxes_iou_threshold
        self.labels_probability_threshold = labels_probability_threshold
        self.suppress_background_boxes = suppress_background_boxes
        self.soft_nms_sigma = soft_nms_sigma_value(soft_nms_sigma)

    def build(self, input_shapes):
        return (None, self.max_number_of_boxes_per_sample, 6)

    def get_config(self):
        return {k: getattr(self, k) for k in (
            'max_number_of_boxes_per_class', 'max_number_of_boxes_per_sample', 'boxes_iou_threshold',
            'labels_probability_threshold', 'suppress_background_boxes', 'soft_nms_sigma')}


def _iou_tf_against(boxes: np.ndarray, k: np.ndarray) -> np.ndarray:
    """TF's NMS IoU of every box (ymin, xmin, ymax, xmax) with box k, in float32 and the kernel's operation order: raw corners,
    no +1, corners swapped where inverted, a degenerate box overlaps nothing"""
    f = np.float32
    y0, x0 = np.minimum(boxes[:, 0], boxes[:, 2]), np.minimum(boxes[:, 1], boxes[:, 3])
    y1, x1 = np.maximum(boxes[:, 0], boxes[:, 2]), np.maximum(boxes[:, 1], boxes[:, 3])
    ky0, kx0, ky1, kx1 = min(k[0], k[2]), min(k[1], k[3]), max(k[0], k[2]), max(k[1], k[3])
    area, area_k = (y1 - y0) * (x1 - x0), f(ky1 - ky0) * f(kx1 - kx0)
    inter = np.maximum(np.minimum(y1, ky1) - np.maximum(y0, ky0), f(0)) * np.maximum(np.minimum(x1, kx1) - np.maximum(x0, kx0), f(0))
    with np.errstate(all="ignore"):
        iou = inter / ((area + area_k) - inter)
    return np.where((area <= 0) | (area_k <= 0), f(0), iou).astype(f)


def soft_nms_reference(corners, probs, max_per_class: int, max_total: int, iou_thr: float, score_thr: float, sigma: float):
    """The definition of ssdseg_combined_nms_soft in NumPy, bit for bit: corners (B, A, 4) = (ymin, xmin, ymax, xmax), probs
    (B, A, C) -> out (B, max_total, 6) = (label, decayed score, xmin, ymin, xmax, ymax) zero padded, valid (B,) int32.

    Per image and class (every class competes, the background too), all in float32 but the weight:
      s_i = probs[i, cls], alive iff s_i > score_thr; at most max_per_class times: pick the alive k of the largest current s (ties:
      lowest anchor), record (s_k, k, cls), kill k; every alive i with iou = IoU(box_i, box_k) dies if iou > iou_thr, otherwise
      s_i = s_i * w and i dies if s_i <= score_thr, with w = float32(exp(-0.5 * x * x / float64(float32(sigma)))), x = float64(iou).
    The picks of all classes are merged by (decayed score desc, anchor asc, class asc) and cut at max_total.
    iou_thr = 1.0 leaves the pure Gaussian Soft-NMS of Bodla et al. (their sigma = 2 * sigma); sigma = 1e30 rounds every w to 1."""
    f = np.float32
    corners, probs = np.asarray(corners, f), np.asarray(probs, f)
    sigma = np.float64(f(soft_nms_sigma_value(sigma, allow_zero=False)))
    iou_thr, score_thr = f(iou_thr), f(score_thr)
    b, a, c = probs.shape
    out, valid = np.zeros((b, max_total, 6), f), np.zeros(b, np.int32)
    for img in range(b):
        picked = []                                               # (decayed score, anchor, class)
        for cls in range(c):
            s = probs[img, :, cls].copy()
            alive = s > score_thr
            for _ in range(max_per_class):
                if not alive.any():
                    break
                k = int(np.argmax(np.where(alive, s, f(-np.inf))))   # the first maximum: the lowest anchor
                picked.append((float(s[k]), k, cls))
                alive[k] = False
                iou = _iou_tf_against(corners[img], corners[img, k])
                alive &= ~(iou > iou_thr)
                x = iou.astype(np.float64)
                with np.errstate(all="ignore"):
                    w = np.exp(-0.5 * x * x / sigma).astype(f)
                s = np.where(alive, s * w, s).astype(f)
                alive &= s > score_thr
        picked.sort(key=lambda t: (-t[0], t[1], t[2]))
        picked = picked[:max_total]
        valid[img] = len(picked)
        for r, (score, i, cls) in enumerate(picked):
            y0, x0, y1, x1 = corners[img, i]
            out[img, r] = (cls, score, x0, y0, x1, y1)
    return out, valid


class SegmentationSuppression(K.Layer):
    """Zero the probabilities of classes the segmentation head did not predict anywhere in the batch
    (reference layers.py:189-212; depth hard-coded to 4 there, quirk Q6)."""
    type_name = "SegmentationSuppression"

    def build(self, input_shapes):
        return input_shapes[1]


class Split(K.Layer):
    """tf.split wrapper (reference layers.py:214-244); only even channel splits are used (models.py:573)."""
    type_name = "Split"

    def __init__(self, num_or_size_splits: Union[int, List[int]], axis: int, num: int = None, **kwargs):
        super().__init__(**kwargs)
        self.num_or_size_splits = num_or_size_splits
        self.axis = axis
        self.num = num

    def build(self, input_shapes):
        s = list(input_shapes[0])
        ax = self.axis % len(s)
        sizes = [s[ax] // self.num_or_size_splits] * self.num_or_size_splits if isinstance(self.num_or_size_splits, int) else list(self.num_or_size_splits)
        assert sum(sizes) == s[ax]
        return [tuple(s[:ax] + [z] + s[ax + 1:]) for z in sizes]

    def get_config(self):
        # the reference's get_config reads a misspelt attribute and would raise (quirk Q9); fixed here
        return {'num_or_size_splits': self.num_or_size_splits, 'axis': self.axis, 'num': self.num}
