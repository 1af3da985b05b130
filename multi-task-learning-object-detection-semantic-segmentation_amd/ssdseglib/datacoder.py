"""Ground-truth encoder / decoder with the reference's API (reference datacoder.py:5-432).

The matching + offset encoding (the hot part: IoU 9600 x G, three-step matching, scatter) runs on the GPU through
ssdseg_encode_targets, for one sample (`read_and_encode`, like the reference's tf.data map) or a whole batch
(`encode_batch`, what the training step uses).  File reading is host glue: CSV via NumPy, PNG via Pillow.

This module is the reference-shaped surface: `DataEncoderDecoder`, `read_image` and the three `augmentation_*` callables with their
three RNG streams.  What the compact hand-over added lives beside it and is re-exported here: the batch containers (`_batches`), the
device-resident training set (`_resident`), the samplers (`_samplers`) and the host specifications of the augmentation kernels
(`_augment_spec`).
"""
import ctypes as C
from typing import Sequence, Tuple

import numpy as np

from ._augment_spec import (_augment_rgb, _crop_gt, _crop_resample, _crop_resample_float, _hsv_to_rgb, _mosaic_gt,      # noqa: F401
                            _mosaic_resample, _rgb_to_hsv)
from ._batches import CompactBatch, Mosaic, ResidentBatch, pad_ground_truth      # noqa: F401
from ._resident import ResidentDataset      # noqa: F401
from ._samplers import _MOSAIC_KEYS, _epoch_plan, _split_crop_options, random_crop_windows, random_mosaic      # noqa: F401

_CORNERS = ("xmin_boxes_default", "ymin_boxes_default", "xmax_boxes_default", "ymax_boxes_default")


def _read_ground_truth(path_file_labels_boxes: str) -> np.ndarray:
    """CSV rows `label,xmin,ymin,xmax,ymax` -> float32 (G, 5)"""
    with open(path_file_labels_boxes, "r", newline="") as f:
        text = f.read().strip()
    rows = [r for r in text.replace("\r\n", "\n").split("\n") if r]
    return np.array([[float(v) for v in r.split(",")] for r in rows], np.float32).reshape(-1, 5)


class DataEncoderDecoder:
    def __init__(self, num_classes: int, image_shape: Tuple[int, int],
                 xmin_boxes_default=None, ymin_boxes_default=None, xmax_boxes_default=None, ymax_boxes_default=None,
                 center_x_boxes_default=None, center_y_boxes_default=None, width_boxes_default=None, height_boxes_default=None,
                 iou_threshold: float = 0.5, standard_deviations_centroids_offsets: Tuple[float, ...] = (0.1, 0.1, 0.2, 0.2),
                 augmentation_horizontal_flip: bool = False) -> None:
        self.num_classes = num_classes
        self.image_height, self.image_width = image_shape
        self.iou_threshold = iou_threshold
        self._stds = tuple(standard_deviations_centroids_offsets)
        (self.standard_deviation_center_x_offsets, self.standard_deviation_center_y_offsets,
         self.standard_deviation_width_offsets, self.standard_deviation_height_offsets) = self._stds
        corners = (xmin_boxes_default, ymin_boxes_default, xmax_boxes_default, ymax_boxes_default)
        centroids = (center_x_boxes_default, center_y_boxes_default, width_boxes_default, height_boxes_default)
        f32 = lambda a: np.asarray(a, dtype=np.float32)
        if all(v is None for v in centroids):
            if any(v is None for v in corners):
                raise ValueError('you must pass all default bounding boxes corners coordinates!')
            xmin, ymin, xmax, ymax = (f32(v) for v in corners)
            cx, cy, w, h = self._coordinates_corners_to_centroids(xmin, ymin, xmax, ymax)
        elif all(v is None for v in corners):
            if any(v is None for v in centroids):
                raise ValueError('you must pass all default bounding boxes centroids coordinates!')
            cx, cy, w, h = (f32(v) for v in centroids)
            xmin, ymin, xmax, ymax = self._coordinates_centroids_to_corners(cx, cy, w, h)
        else:
            # passing both sets is rejected, exactly like the reference (its "both" branch is unreachable: quirk Q5)
            raise ValueError('you must pass all default bounding boxes centroids coordinates, or corners coordinates or both!')
        self.xmin_boxes_default, self.ymin_boxes_default, self.xmax_boxes_default, self.ymax_boxes_default = xmin, ymin, xmax, ymax
        self.center_x_boxes_default, self.center_y_boxes_default, self.width_boxes_default, self.height_boxes_default = cx, cy, w, h
        self.boxes_area_default = ((ymax - ymin + 1.0) * (xmax - xmin + 1.0))[:, None]
        self.augmentation_horizontal_flip = augmentation_horizontal_flip
        self._rng = np.random.default_rng(1993)
        self._dev = None

    # ---- coordinate helpers (reference datacoder.py:119-175)
    @staticmethod
    def _coordinates_corners_to_centroids(xmin, ymin, xmax, ymax):
        return (xmax + xmin) / 2.0, (ymax + ymin) / 2.0, xmax - xmin + 1.0, ymax - ymin + 1.0

    @staticmethod
    def _coordinates_centroids_to_corners(center_x, center_y, width, height):
        return center_x - (width - 1.0) / 2.0, center_y - (height - 1.0) / 2.0, center_x + (width - 1.0) / 2.0, center_y + (height - 1.0) / 2.0

    def _corners(self) -> np.ndarray:
        """the default boxes as the encode kernel takes them: float32 (A, 4) = (xmin, ymin, xmax, ymax)"""
        return np.stack([getattr(self, name) for name in _CORNERS], axis=1).astype(np.float32)

    # ---- GPU encode
    def _device_anchors(self):
        if self._dev is None:
            from . import _engine
            ctx = _engine.default_context()
            self._dev = (ctx, ctx.array(self._corners()))
        return self._dev

    def encode_batch(self, labels_boxes: Sequence[np.ndarray], to_host: bool = True):
        """labels_boxes: per image an array (G, 5) = (label, xmin, ymin, xmax, ymax).
        -> labels (B, A, num_classes) one-hot, boxes (B, A, 4) offsets (NumPy, or DeviceBuffers with to_host=False)."""
        ctx, anchors = self._device_anchors()
        b = len(labels_boxes)
        gmax = max(1, max((np.asarray(g).reshape(-1, 5).shape[0] for g in labels_boxes), default=1))       # no cap: as many as there are
        gt, cnt = pad_ground_truth(labels_boxes, gmax)
        a = anchors.shape[0]
        labels, boxes = ctx.empty((b, a, self.num_classes)), ctx.empty((b, a, 4))
        ctx.call("ssdseg_encode_targets", anchors, a, ctx.array(gt), ctx.array(cnt), b, gmax, self.num_classes, float(self.iou_threshold),
                 (C.c_float * 4)(*self._stds), labels, boxes, None)
        if to_host:
            return labels.download(), boxes.download()
        return labels, boxes

    def _flip_boxes(self, gt: np.ndarray) -> np.ndarray:
        """x -> W - x, with W the image width, NOT W-1 (quirk Q8, reference datacoder.py:203)"""
        out = gt.copy()
        out[:, 1], out[:, 3] = self.image_width - gt[:, 3], self.image_width - gt[:, 1]
        return out

    def _draw_flip(self) -> bool:
        """one sample's flip (reference datacoder.py:337): a draw from the encoder's stream only when the augmentation is on"""
        return bool(self.augmentation_horizontal_flip and self._rng.uniform(0, 1) >= 0.5)

    def _encode_ground_truth_labels_boxes(self, path_file_labels_boxes: str, augment_with_horizontal_flip: bool):
        """CSV rows `label,xmin,ymin,xmax,ymax` -> (labels (A, C), boxes (A, 4)) (reference datacoder.py:177-300)."""
        gt = _read_ground_truth(path_file_labels_boxes)
        if augment_with_horizontal_flip:
            gt = self._flip_boxes(gt)
        labels, boxes = self.encode_batch([gt])
        return labels[0], boxes[0]

    def read_and_encode(self, path_file_image: str, path_file_mask: str, path_file_labels_boxes: str):
        """(image, {'output-mask', 'output-labels', 'output-boxes'}) for one sample (reference datacoder.py:302-347)."""
        image = read_image(path_file_image)
        from PIL import Image
        mask_idx = np.asarray(Image.open(path_file_mask).convert("L"), np.int64)
        mask = np.eye(self.num_classes, dtype=np.float32)[np.clip(mask_idx, 0, self.num_classes - 1)]
        mask[mask_idx >= self.num_classes] = 0.0        # tf.one_hot gives an all-zero row for out-of-range indices
        flip = self._draw_flip()
        if flip:
            image, mask = image[:, ::-1].copy(), mask[:, ::-1].copy()
        labels, boxes = self._encode_ground_truth_labels_boxes(path_file_labels_boxes, flip)
        return image, {'output-mask': mask, 'output-labels': labels, 'output-boxes': boxes}

    # ---- compact hand-over: what the files hold goes to the GPU, the expansion happens there (csrc/inputs.hip)
    def read_compact(self, path_file_image: str, path_file_mask: str, path_file_labels_boxes: str):
        """one sample as (uint8 image (H, W, 3), uint8 class-index mask (H, W), ground truth (G, 5), flip flag): the inputs of
        read_and_encode before its float expansion (reference datacoder.py:325-345); `compact_batch` stacks them"""
        from PIL import Image
        image = np.asarray(Image.open(path_file_image).convert("RGB"), np.uint8)
        mask_idx = np.asarray(Image.open(path_file_mask).convert("L"), np.uint8)
        return image, mask_idx, _read_ground_truth(path_file_labels_boxes), self._draw_flip()

    def compact_batch(self, samples) -> CompactBatch:
        images, masks, gts, flips = zip(*samples)
        return CompactBatch(np.stack(images), np.stack(masks), list(gts), np.asarray(flips, np.uint8), self)

    # ---- decode of GROUND-TRUTH offsets (reference datacoder.py:349-432)
    def decode_to_centroids(self, offsets_centroids, output_decoded_centroids_separately: bool = False):
        o = np.asarray(offsets_centroids, np.float32)
        sx, sy, sw, sh = (np.float32(s) for s in self._stds)
        not_background = (np.abs(o).sum(axis=-1) > 0.0).astype(np.float32)
        center_x = (o[:, 0] * sx * self.width_boxes_default + self.center_x_boxes_default) * not_background
        center_y = (o[:, 1] * sy * self.height_boxes_default + self.center_y_boxes_default) * not_background
        width = (np.exp(o[:, 2] * sw) - 1.0).astype(np.float32) * self.width_boxes_default * not_background
        height = (np.exp(o[:, 3] * sh) - 1.0).astype(np.float32) * self.height_boxes_default * not_background
        if output_decoded_centroids_separately:
            return center_x, center_y, width, height
        return np.stack([center_x, center_y, width, height], axis=1)

    def decode_to_corners(self, offsets_centroids, output_decoded_corners_separately: bool = False):
        center_x, center_y, width, height = self.decode_to_centroids(offsets_centroids, True)
        xmin, ymin, xmax, ymax = self._coordinates_centroids_to_corners(center_x, center_y, width, height)
        not_background = ((np.abs(center_x) + np.abs(center_y) + np.abs(width) + np.abs(height)) > 0.0).astype(np.float32)
        xmin, ymin, xmax, ymax = xmin * not_background, ymin * not_background, xmax * not_background, ymax * not_background
        if output_decoded_corners_separately:
            return xmin, ymin, xmax, ymax
        return np.stack([xmin, ymin, xmax, ymax], axis=1)


# ---- the augmentation callables of the reference's `.map(...)` chain, each with a stream of its own: the colour draws of _aug_rng
# are not disturbed by the crop windows, nor either of them by the mosaics
_aug_rng = np.random.default_rng(1993)
_crop_rng = np.random.default_rng(1993)
_mosaic_rng = np.random.default_rng(1993)


def augmentation_random_crop(image_batch, targets_batch=None, **options):
    """random zoom-in crops / zoom-out expansions for a CompactBatch: returns (a new CompactBatch sharing its arrays, with one freshly
    drawn window per sample attached, targets_batch), the analogue of augmentation_rgb_channels on a compact batch.  options: the
    keywords of random_crop_windows plus `fill` (r, g, b) and `fill_class`.  The loader applies the windows on the GPU
    (ssdseg_crop_inputs, ssdseg_crop_gt) before the flip and the colour step.  Float (images, targets) batches are refused: their
    anchors are already encoded and cannot be re-cropped.  fill_class=255 (any index >= 4) is the void fill: the padding of a
    zoom-out becomes all-zero one-hot rows, which `cross_entropy` ignores as it stands and the other mask losses and the mask metric
    ignore with `ignore_void=True`; the default 0 labels the padding as background."""
    if not isinstance(image_batch, CompactBatch):
        raise ValueError("augmentation_random_crop takes a CompactBatch: a float (images, targets) batch holds encoded anchors that "
                         "cannot be re-cropped")
    cb = image_batch
    kw, fill = _split_crop_options(options)
    windows = random_crop_windows(_crop_rng, len(cb), cb.images.shape[1], cb.images.shape[2], **kw)
    return cb.replace(crop_windows=windows, crop_fill=fill), targets_batch


def augmentation_mosaic(image_batch, targets_batch=None, **options):
    """a random mosaic for a CompactBatch: returns (a new CompactBatch sharing its arrays, with a freshly drawn Mosaic over its own
    samples attached, targets_batch), the analogue of augmentation_random_crop.  options: the keywords of random_mosaic plus `fill`
    (r, g, b) and `fill_class`.  The loader assembles the images on the GPU (ssdseg_mosaic_inputs, ssdseg_mosaic_gt) before the flip
    and the colour step.  Float (images, targets) batches are refused: their anchors are already encoded.  fill_class=255 is the void
    fill, as in augmentation_random_crop."""
    if not isinstance(image_batch, CompactBatch):
        raise ValueError("augmentation_mosaic takes a CompactBatch: a float (images, targets) batch holds encoded anchors that cannot "
                         "be reassembled")
    cb = image_batch
    kw, fill = _split_crop_options(options, "mosaic", _MOSAIC_KEYS)
    mosaic = random_mosaic(_mosaic_rng, len(cb), cb.images.shape[1], cb.images.shape[2], **kw)
    return cb.replace(mosaic=mosaic, mosaic_fill=fill), targets_batch


def _draw_rgb():
    """one draw set of augmentation_rgb_channels (reference datacoder.py:452-461): (hue_delta, saturation_factor, contrast_factor,
    brightness_delta)"""
    return (_aug_rng.uniform(-0.05, 0.05), _aug_rng.uniform(0.95, 1.05), _aug_rng.uniform(0.90, 1.10), _aug_rng.uniform(-0.10, 0.10))


def augmentation_rgb_channels(image_batch, targets_batch):
    """random hue (+-0.05), saturation (0.95..1.05), contrast (0.9..1.1), brightness (+-0.10) then clip to [0, 255]
    (reference datacoder.py:452-464; the deltas are the [0,1]-scale ones applied to 0..255 images, quirk Q11).
    One draw set per call, like tf.image.random_* on a 4-D batch; TF's exact RNG streams are not reproduced.
    Float arrays: applied here, on the host (_augment_rgb).  A CompactBatch: returns a new CompactBatch sharing its arrays with the
    draws attached; the loader applies them on the GPU (ssdseg_rgb_augment) when it expands the batch."""
    draws = _draw_rgb()
    if isinstance(image_batch, CompactBatch):
        return image_batch.replace(rgb_draws=draws), targets_batch
    return _augment_rgb(image_batch, *draws), targets_batch


def read_image(path_file_image: str) -> np.ndarray:
    """PNG -> float32 (H, W, 3) in 0..255 (reference datacoder.py:468-484)."""
    from PIL import Image
    return np.asarray(Image.open(path_file_image).convert("RGB"), np.float32)
