"""Training metrics with the reference's factory API (reference metrics.py:5-220): each factory returns
`metric(y_true, y_pred) -> (batch,)`, computed by the HIP kernels `ssdseg_metric_*`.

The returned callables carry `metric_kind` and their parameters, so `Model.compile(metrics={output: fn})` can evaluate them
inside the train / validation step straight from the device buffers of that step (the segmentation metric from the
low-resolution logits: `output-mask` is never materialised while training).  Called directly they accept host arrays
(uploaded) or device buffers.  Semantics follow the reference to the letter:
  * jaccard_iou_segmentation_masks_metric is the SOFT Jaccard on probabilities (no arg-max), epsilon in the denominator;
  * categorical_accuracy_metric counts equal(one_hot(argmax p), y_true) per class over ALL boxes (agreeing zeros count);
  * jaccard_iou_bounding_boxes_metric keeps the reference's decode conventions and is NaN for images without objects.
"""
from typing import Callable, List

import numpy as np

from .losses import OUT, _ctx, boxes_on_context, c4, dev, per_sample, shape_of, void_flag


def jaccard_iou_segmentation_masks(classes_weights: List[float], ignore_void: bool = False) -> Callable:
    """reference metrics.py:5-50.  ignore_void=True: total = sum (t + p) over the labelled pixels only (a pixel whose y_true row
    is all zero is void), as the mask losses' option of the same name."""
    if len(classes_weights) != 4:
        raise ValueError("the segmentation metric kernel handles the reference's 4 classes (background + 3)")
    cw = c4(classes_weights)
    entry = "ssdseg_metric_mask_iou_void" if void_flag(ignore_void) else "ssdseg_metric_mask_iou"

    def jaccard_iou_segmentation_masks_metric(y_true, y_pred):
        n, h, w, c = shape_of(y_pred)
        return per_sample(entry, n, dev(y_pred), n, h, w, c, 1, 1, 0, dev(y_true), cw, OUT)

    f = jaccard_iou_segmentation_masks_metric
    f.metric_kind, f.classes_weights, f._cw = "mask_iou", tuple(float(x) for x in classes_weights), cw
    f.ignore_void = bool(ignore_void)
    return f


def jaccard_iou_bounding_boxes(center_x_boxes_default, center_y_boxes_default, width_boxes_default, height_boxes_default,
                               standard_deviations_centroids_offsets) -> Callable:
    """reference metrics.py:53-173"""
    anchors = np.ascontiguousarray(np.stack([np.asarray(v, np.float32).reshape(-1) for v in
                                             (center_x_boxes_default, center_y_boxes_default, width_boxes_default, height_boxes_default)], axis=1))
    stds, anchors_on = c4(standard_deviations_centroids_offsets), boxes_on_context(anchors)

    def jaccard_iou_bounding_boxes_metric(y_true, y_pred):
        b, a = shape_of(y_pred)[:2]
        if a != anchors.shape[0]:
            raise ValueError(f"{a} boxes per image, {anchors.shape[0]} default boxes")
        return per_sample("ssdseg_metric_box_iou", b, dev(y_true), dev(y_pred), anchors_on(_ctx()), stds, b, a, OUT)

    f = jaccard_iou_bounding_boxes_metric
    f.metric_kind, f.anchors_on, f._stds = "box_iou", anchors_on, stds
    return f


def categorical_accuracy(classes_weights: List[float]) -> Callable:
    """reference metrics.py:176-220"""
    if len(classes_weights) != 4:
        raise ValueError("the label metric kernel handles the reference's 4 classes (background + 3)")
    cw = c4(classes_weights)

    def categorical_accuracy_metric(y_true, y_pred):
        b, a, c = shape_of(y_pred)
        return per_sample("ssdseg_metric_label_accuracy", b, dev(y_true), dev(y_pred), b, a, c, cw, OUT)

    f = categorical_accuracy_metric
    f.metric_kind, f.classes_weights, f._cw = "label_accuracy", tuple(float(x) for x in classes_weights), cw
    return f
