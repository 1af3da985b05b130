"""Ground-truth encoder / decoder with the reference's API (reference datacoder.py:5-432).

The matching + offset encoding (the hot part: IoU 9600 x G, three-step matching, scatter) runs on the GPU through
ssdseg_encode_targets, for one sample (`read_and_encode`, like the reference's tf.data map) or a whole batch
(`encode_batch`, what the training step uses).  File reading is host glue: CSV via NumPy, PNG via Pillow.
"""
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

_CORNERS = ("xmin_boxes_default", "ymin_boxes_default", "xmax_boxes_default", "ymax_boxes_default")
_CENTROIDS = ("center_x_boxes_default", "center_y_boxes_default", "width_boxes_default", "height_boxes_default")


class DataEncoderDecoder:
    def __init__(self, num_classes: int, image_shape: Tuple[int, int],
                 xmin_boxes_default=None, ymin_boxes_default=None, xmax_boxes_default=None, ymax_boxes_default=None,
                 center_x_boxes_default=None, center_y_boxes_default=None, width_boxes_default=None, height_boxes_default=None,
                 iou_threshold: float = 0.5, standard_deviations_centroids_offsets: Tuple[float, ...] = (0.1, 0.1, 0.2, 0.2),
                 augmentation_horizontal_flip: bool = False) -> None:
        self.num_classes = num_classes
        self.image_height, self.image_width = image_shape
        self.iou_threshold = iou_threshold
        (self.standard_deviation_center_x_offsets, self.standard_deviation_center_y_offsets,
         self.standard_deviation_width_offsets, self.standard_deviation_height_offsets) = standard_deviations_centroids_offsets
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

    @property
    def _stds(self):
        return (self.standard_deviation_center_x_offsets, self.standard_deviation_center_y_offsets,
                self.standard_deviation_width_offsets, self.standard_deviation_height_offsets)

    # ---- GPU encode
    def _device_anchors(self):
        if self._dev is None:
            from . import _engine
            ctx = _engine.default_context()
            corners = np.stack([self.xmin_boxes_default, self.ymin_boxes_default, self.xmax_boxes_default, self.ymax_boxes_default], axis=1)
            self._dev = (ctx, ctx.array(corners.astype(np.float32)))
        return self._dev

    def encode_batch(self, labels_boxes: Sequence[np.ndarray], to_host: bool = True):
        """labels_boxes: per image an array (G, 5) = (label, xmin, ymin, xmax, ymax).
        -> labels (B, A, num_classes) one-hot, boxes (B, A, 4) offsets (NumPy, or DeviceBuffers with to_host=False)."""
        ctx, anchors = self._device_anchors()
        b = len(labels_boxes)
        gmax = max(1, max((np.asarray(g).reshape(-1, 5).shape[0] for g in labels_boxes), default=1))
        gt = np.zeros((b, gmax, 5), np.float32)
        cnt = np.zeros(b, np.int32)
        for i, g in enumerate(labels_boxes):
            g = np.asarray(g, np.float32).reshape(-1, 5)
            gt[i, :g.shape[0]] = g
            cnt[i] = g.shape[0]
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

    def _encode_ground_truth_labels_boxes(self, path_file_labels_boxes: str, augment_with_horizontal_flip: bool):
        """CSV rows `label,xmin,ymin,xmax,ymax` -> (labels (A, C), boxes (A, 4)) (reference datacoder.py:177-300)."""
        with open(path_file_labels_boxes, "r", newline="") as f:
            text = f.read().strip()
        rows = [r for r in text.replace("\r\n", "\n").split("\n") if r]
        gt = np.array([[float(v) for v in r.split(",")] for r in rows], np.float32).reshape(-1, 5)
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
        flip = bool(self.augmentation_horizontal_flip and self._rng.uniform(0, 1) >= 0.5)
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
        with open(path_file_labels_boxes, "r", newline="") as f:
            text = f.read().strip()
        rows = [r for r in text.replace("\r\n", "\n").split("\n") if r]
        gt = np.array([[float(v) for v in r.split(",")] for r in rows], np.float32).reshape(-1, 5)
        flip = bool(self.augmentation_horizontal_flip and self._rng.uniform(0, 1) >= 0.5)
        return image, mask_idx, gt, flip

    def compact_batch(self, samples) -> "CompactBatch":
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


class CompactBatch:
    """A training batch as the files hold it: uint8 pixels (B, H, W, 3), uint8 class indices (B, H, W), per-sample ground-truth
    rows (label, xmin, ymin, xmax, ymax) and flip flags -- 39 MB instead of the 285 MB of float32 tensors at batch 32, 480x640.
    `Model.fit` / `train_on_batch` accept it in place of (images, targets): float conversion, one-hot, mirroring and the anchor
    encoding run on the GPU (ssdseg_expand_inputs, ssdseg_flip_gt_boxes, ssdseg_encode_targets).  `augmentation_rgb_channels(cb,
    targets)` returns a copy carrying one colour-augmentation draw set (`rgb_draws`), applied on the GPU too (ssdseg_rgb_augment)."""

    def __init__(self, images_u8, mask_index_u8, ground_truth, flip, encoder: "DataEncoderDecoder", rgb_draws=None):
        self.images = np.ascontiguousarray(images_u8, np.uint8)
        self.mask_index = np.ascontiguousarray(mask_index_u8, np.uint8)
        if self.images.ndim != 4 or self.images.shape[-1] != 3 or self.mask_index.shape != self.images.shape[:3]:
            raise ValueError(f"compact batch: images {self.images.shape} must be (B, H, W, 3) and masks {self.mask_index.shape} (B, H, W)")
        self.ground_truth = [np.asarray(g, np.float32).reshape(-1, 5) for g in ground_truth]
        if len(self.ground_truth) != self.images.shape[0]:
            raise ValueError("compact batch: one ground-truth array per image")
        self.flip = None if flip is None else np.ascontiguousarray(flip, np.uint8).reshape(self.images.shape[0])
        self.encoder = encoder
        # (hue_delta, saturation_factor, contrast_factor, brightness_delta) of augmentation_rgb_channels, applied on the device
        # (ssdseg_rgb_augment) when the batch is expanded; None: the pixels go in as they are
        self.rgb_draws = _check_rgb_draws(rgb_draws)

    def __len__(self):
        return self.images.shape[0]


def _check_rgb_draws(draws):
    if draws is None:
        return None
    try:
        out = tuple(float(v) for v in draws)
    except (TypeError, ValueError):
        raise ValueError(f"rgb_draws must be None or four finite numbers, got {draws!r}") from None
    if len(out) != 4 or not all(np.isfinite(out)):
        raise ValueError(f"rgb_draws must be None or four finite numbers (hue, saturation, contrast, brightness), got {draws!r}")
    return out


_aug_rng = np.random.default_rng(1993)


def _draw_rgb():
    """one draw set of augmentation_rgb_channels (reference datacoder.py:452-461): (hue_delta, saturation_factor, contrast_factor,
    brightness_delta)"""
    return (_aug_rng.uniform(-0.05, 0.05), _aug_rng.uniform(0.95, 1.05), _aug_rng.uniform(0.90, 1.10), _aug_rng.uniform(-0.10, 0.10))


def _rgb_to_hsv(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    mx, mn = rgb.max(-1), rgb.min(-1)
    d = mx - mn
    s = np.where(mx > 0, d / np.where(mx > 0, mx, 1), 0)
    dd = np.where(d > 0, d, 1)
    h = np.where(mx == r, (g - b) / dd, np.where(mx == g, 2.0 + (b - r) / dd, 4.0 + (r - g) / dd))
    h = np.where(d > 0, (h / 6.0) % 1.0, 0.0)
    return np.stack([h, s, mx], -1)


def _hsv_to_rgb(hsv):
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    dh = h * 6.0
    k = lambda n: (n + dh) % 6.0
    f = lambda n: v - v * s * np.clip(np.minimum(k(n), 4.0 - k(n)), 0.0, 1.0)
    return np.stack([f(5), f(3), f(1)], -1)


def _augment_rgb(x, hue_delta, saturation_factor, contrast_factor, brightness_delta):
    """the four adjustments with GIVEN random draws (tf.image.adjust_hue / adjust_saturation / adjust_contrast /
    adjust_brightness on float images, then the clip of reference datacoder.py:464)"""
    x = np.asarray(x, np.float32)
    hsv = _rgb_to_hsv(x)
    hsv[..., 0] = (hsv[..., 0] + hue_delta) % 1.0
    x = _hsv_to_rgb(hsv)
    hsv = _rgb_to_hsv(x)
    hsv[..., 1] = np.clip(hsv[..., 1] * saturation_factor, 0.0, 1.0)
    x = _hsv_to_rgb(hsv)
    mean = x.mean(axis=(1, 2), keepdims=True)          # per image and channel
    x = (x - mean) * contrast_factor + mean
    x = x + brightness_delta
    return np.clip(x, 0.0, 255.0).astype(np.float32)


def augmentation_rgb_channels(image_batch, targets_batch):
    """random hue (+-0.05), saturation (0.95..1.05), contrast (0.9..1.1), brightness (+-0.10) then clip to [0, 255]
    (reference datacoder.py:452-464; the deltas are the [0,1]-scale ones applied to 0..255 images, quirk Q11).
    One draw set per call, like tf.image.random_* on a 4-D batch; TF's exact RNG streams are not reproduced.
    Float arrays: applied here, on the host (_augment_rgb).  A CompactBatch: returns a new CompactBatch sharing its arrays with the
    draws attached; the loader applies them on the GPU (ssdseg_rgb_augment) when it expands the batch."""
    draws = _draw_rgb()
    if isinstance(image_batch, CompactBatch):
        cb = image_batch
        return CompactBatch(cb.images, cb.mask_index, cb.ground_truth, cb.flip, cb.encoder, rgb_draws=draws), targets_batch
    return _augment_rgb(image_batch, *draws), targets_batch


# ---- device-resident training set: NB03#cell8's shuffle / map(read_and_encode) / batch / map(augmentation) chain per epoch
_RGB_RANGES = ((-0.05, 0.05), (0.95, 1.05), (0.90, 1.10), (-0.10, 0.10))     # the ranges of _draw_rgb (reference datacoder.py:452-461)


def _epoch_plan(rng, num_samples: int, batch_size: int, shuffle: bool, flip: bool, rgb_augmentation: bool, drop_remainder: bool):
    """One epoch of the reference's input chain as host lists, no device access: [(index int32 (b,), flip uint8 (b,) or None,
    rgb draws (4 floats) or None)].  A fresh uniform permutation of the SAMPLES (`.shuffle(buffer_size=len)`), a fresh flip draw
    per sample (`uniform >= 0.5`, reference datacoder.py:337-345), batches cut afterwards with the last partial one kept unless
    drop_remainder, one colour draw set per batch (`.batch(B).map(augmentation_rgb_channels)`)."""
    order = rng.permutation(num_samples) if shuffle else np.arange(num_samples)
    order = order.astype(np.int32)
    flips = (rng.uniform(0.0, 1.0, num_samples) >= 0.5).astype(np.uint8) if flip else None
    plan = []
    for lo in range(0, num_samples, batch_size):
        hi = min(lo + batch_size, num_samples)
        if drop_remainder and hi - lo < batch_size:
            break
        draws = tuple(float(rng.uniform(a, b)) for a, b in _RGB_RANGES) if rgb_augmentation else None
        plan.append((order[lo:hi].copy(), None if flips is None else flips[lo:hi].copy(), draws))
    return plan


class ResidentBatch:
    """A batch of a ResidentDataset: which samples (`index`, int32), which of them mirrored (`flip`, uint8 or None) and the colour
    draws (`rgb_draws` or None) -- a few host bytes; the pixels stay on the device.  `Model.fit` / `train_on_batch` accept it."""

    def __init__(self, dataset: "ResidentDataset", index, flip=None, rgb_draws=None):
        self.dataset = dataset
        self.index = np.ascontiguousarray(index, np.int32).reshape(-1)
        if self.index.size == 0:
            raise ValueError("resident batch: no samples")
        if self.index.min() < 0 or self.index.max() >= dataset.num_samples:
            raise IndexError(f"resident batch: sample index outside [0, {dataset.num_samples})")
        self.flip = None if flip is None else np.ascontiguousarray(flip, np.uint8).reshape(-1)
        if self.flip is not None and self.flip.size != self.index.size:
            raise ValueError("resident batch: one flip flag per sample")
        self.rgb_draws = _check_rgb_draws(rgb_draws)

    @property
    def encoder(self):
        return self.dataset.encoder

    def __len__(self):
        return int(self.index.size)


class ResidentDataset:
    """A training set kept in device memory as the files hold it -- uint8 pixels, uint8 class indices, ground-truth rows: 1.2 MB per
    480x640 sample -- uploaded once.  Iterating it is ONE EPOCH of the reference's chain (NB03#cell8:
    `.shuffle(len).map(read_and_encode).batch(B).map(augmentation_rgb_channels)`): a new permutation of the samples, a new flip
    draw per sample when `encoder.augmentation_horizontal_flip`, one colour draw set per batch when `rgb_augmentation`, the last
    partial batch kept unless `drop_remainder` -- all from the dataset's own Generator(seed); TF's RNG streams are not reproduced.
    The batches are `ResidentBatch` objects: `Model.fit(ds, epochs=N)` builds each one on the device (ssdseg_gather_inputs,
    ssdseg_gather_gt, ssdseg_encode_targets), so after the upload no pixel crosses PCIe and the host does no per-sample work.
    `samples`: an iterable of `read_compact` tuples (their flip flag is ignored); `capacity`: slots to allocate (default: the number
    of samples), filled with `append` / `write` without holding the set on the host."""

    GMAX = 64       # ground-truth rows per sample, as the compact loader (the encode kernel holds them in LDS)

    def __init__(self, encoder: "DataEncoderDecoder", samples=None, *, capacity: Optional[int] = None, batch_size: int = 16,
                 shuffle: bool = True, rgb_augmentation: bool = False, drop_remainder: bool = False, seed=None):
        samples = list(samples) if samples is not None else []
        capacity = len(samples) if capacity is None else int(capacity)
        if capacity <= 0 or capacity < len(samples):
            raise ValueError(f"resident dataset: capacity {capacity} for {len(samples)} samples")
        if int(batch_size) <= 0:
            raise ValueError("resident dataset: batch_size must be positive")
        self.encoder = encoder
        self.capacity, self.batch_size = capacity, int(batch_size)
        self.shuffle, self.rgb_augmentation, self.drop_remainder = bool(shuffle), bool(rgb_augmentation), bool(drop_remainder)
        self.height, self.width = int(encoder.image_height), int(encoder.image_width)
        self.num_samples = 0
        self._rng = np.random.default_rng(seed)
        self.ctx = self.images = self.masks = self.gt = self.cnt = None
        self._gt_labels = {}      # slot -> the labels of its ground-truth rows (int32): what evaluation counts per class on the host
        for sample in samples:
            self.append(*sample[:3])

    def _allocate(self) -> None:
        """the four pools, on the first write (planning an epoch needs no device)"""
        from . import _engine
        self.ctx = ctx = _engine.default_context()
        self.images = ctx.empty((self.capacity, self.height, self.width, 3), np.uint8)
        self.masks = ctx.empty((self.capacity, self.height, self.width), np.uint8)
        self.gt = ctx.empty((self.capacity, self.GMAX, 5))
        self.cnt = ctx.empty(self.capacity, np.int32)

    def write(self, slot: int, image_u8, mask_u8, gt) -> None:
        """sample `slot` <- (uint8 image (H, W, 3), uint8 class-index mask (H, W), ground truth (G, 5)); slots up to the highest one
        written count as samples"""
        slot = int(slot)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"resident dataset: slot {slot} outside [0, {self.capacity})")
        image = np.ascontiguousarray(image_u8, np.uint8)
        mask = np.ascontiguousarray(mask_u8, np.uint8)
        if image.shape != (self.height, self.width, 3) or mask.shape != (self.height, self.width):
            raise ValueError(f"resident dataset: image {image.shape} / mask {mask.shape} for samples of {self.height}x{self.width}")
        g = np.asarray(gt, np.float32).reshape(-1, 5)
        if g.shape[0] > self.GMAX:
            raise ValueError(f"more than {self.GMAX} ground-truth boxes in one image")
        rows = np.zeros((self.GMAX, 5), np.float32)
        rows[:g.shape[0]] = g
        if self.images is None:
            self._allocate()
        hw = self.height * self.width
        self.images.view(slot * hw * 3, image.shape).upload(image)
        self.masks.view(slot * hw, mask.shape).upload(mask)
        self.gt.view(slot * self.GMAX * 5, rows.shape).upload(rows)
        self.cnt.view(slot, (1,)).upload(np.array([g.shape[0]], np.int32))
        self._gt_labels[slot] = g[:, 0].astype(np.int32)
        self.num_samples = max(self.num_samples, slot + 1)

    def append(self, image_u8, mask_u8, gt) -> int:
        slot = self.num_samples
        self.write(slot, image_u8, mask_u8, gt)
        return slot

    def __len__(self):
        """batches per epoch"""
        n, b = self.num_samples, self.batch_size
        return n // b if self.drop_remainder else -(-n // b)

    def batch(self, index, flip=None, rgb_draws=None) -> ResidentBatch:
        """an explicit batch: these samples, mirrored where flagged, with these colour draws"""
        return ResidentBatch(self, index, flip, rgb_draws)

    def __iter__(self):
        plan = _epoch_plan(self._rng, self.num_samples, self.batch_size, self.shuffle, bool(self.encoder.augmentation_horizontal_flip),
                           self.rgb_augmentation, self.drop_remainder)
        return iter([ResidentBatch(self, index, flip, draws) for index, flip, draws in plan])

    def to_compact(self, batch: ResidentBatch) -> CompactBatch:
        """the named samples downloaded into an equal CompactBatch (same flips, same draws): for debugging and tests"""
        hw = self.height * self.width
        images = np.stack([self.images.view(int(i) * hw * 3, (self.height, self.width, 3)).download() for i in batch.index])
        masks = np.stack([self.masks.view(int(i) * hw, (self.height, self.width)).download() for i in batch.index])
        cnt = self.cnt.download()
        gts = [self.gt.view(int(i) * self.GMAX * 5, (self.GMAX, 5)).download()[:cnt[i]] for i in batch.index]
        flip = np.zeros(len(batch), np.uint8) if batch.flip is None else batch.flip.copy()
        return CompactBatch(images, masks, gts, flip, self.encoder, rgb_draws=batch.rgb_draws)


def read_image(path_file_image: str) -> np.ndarray:
    """PNG -> float32 (H, W, 3) in 0..255 (reference datacoder.py:468-484)."""
    from PIL import Image
    return np.asarray(Image.open(path_file_image).convert("RGB"), np.float32)
