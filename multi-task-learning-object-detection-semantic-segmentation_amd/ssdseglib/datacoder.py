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
    targets)` returns a copy carrying one colour-augmentation draw set (`rgb_draws`), applied on the GPU too (ssdseg_rgb_augment);
    `augmentation_random_crop(cb, targets)` one carrying a crop window per sample (`crop_windows`, `crop_fill` = (r, g, b,
    fill_class)), applied on the GPU in front of the flip and the colour step (ssdseg_crop_inputs, ssdseg_crop_gt);
    `augmentation_mosaic(cb, targets)` one carrying a `Mosaic` (`mosaic`, `mosaic_fill` = (r, g, b, fill_class)) whose sources are
    positions within this batch, applied on the GPU in the crop's place (ssdseg_mosaic_inputs, ssdseg_mosaic_gt).  A batch carries
    crop windows or a mosaic, not both."""

    def __init__(self, images_u8, mask_index_u8, ground_truth, flip, encoder: "DataEncoderDecoder", rgb_draws=None, *, crop_windows=None,
                 crop_fill=None, mosaic=None, mosaic_fill=None):
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
        # one crop window (x0, y0, w, h) per sample and (r, g, b, fill_class) for what lies outside the image, applied on the
        # device (ssdseg_crop_inputs / ssdseg_crop_gt) BEFORE the flip and the colour step; None: no crop
        self.crop_windows = _check_crop_windows(crop_windows, self.images.shape[0], self.images.shape[1], self.images.shape[2])
        self.crop_fill = _check_crop_fill(crop_fill)
        # four (source position within this batch, window) pairs per sample around a split point, and the fill, applied on the device
        # (ssdseg_mosaic_inputs / ssdseg_mosaic_gt) in the crop's place; None: no mosaic
        self.mosaic = _check_mosaic(mosaic, self.crop_windows, self.images.shape[0], self.images.shape[1], self.images.shape[2])
        self.mosaic_fill = _check_crop_fill(mosaic_fill, "mosaic_fill")

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


def _check_crop_windows(windows, b: int, height: int, width: int):
    """None, or (b, 4) float32 windows (x0, y0, w, h): finite and inside the range the C-ABI takes (include/ssdseg.h)"""
    if windows is None:
        return None
    try:
        out = np.ascontiguousarray(windows, np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"crop_windows must be None or a ({b}, 4) array of numbers, got {windows!r}") from None
    if out.shape != (b, 4):
        raise ValueError(f"crop_windows must be None or one (x0, y0, w, h) per sample, shape ({b}, 4), got {out.shape}")
    if not np.isfinite(out).all():
        raise ValueError("crop_windows must be finite")
    if not _windows_in_range(out, height, width):
        raise ValueError(f"crop_windows: need 1 <= w <= {16 * width}, 1 <= h <= {16 * height}, |x0| <= {16 * width}, |y0| <= {16 * height}")
    return out


def _windows_in_range(windows, height: int, width: int) -> bool:
    """float32 windows (..., 4) = (x0, y0, w, h): |x0| <= 16 W, |y0| <= 16 H, 1 <= w <= 16 W, 1 <= h <= 16 H (a NaN is outside)"""
    limit = np.array([16 * width, 16 * height, 16 * width, 16 * height], np.float32)
    return bool((np.abs(windows) <= limit).all() and (windows[..., 2:] >= 1).all())


def _check_crop_fill(fill, name="crop_fill"):
    """None, or (r, g, b, fill_class): four integers in 0..255"""
    if fill is None:
        return None
    try:
        out = tuple(int(v) for v in fill)
        exact = all(float(v) == float(o) for v, o in zip(fill, out))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be None or four integers (r, g, b, fill_class), got {fill!r}") from None
    if len(out) != 4 or not exact or not all(0 <= v <= 255 for v in out):
        raise ValueError(f"{name} must be None or four integers in 0..255 (r, g, b, fill_class), got {fill!r}")
    return out


# ---- random crop / zoom-out: the host spec of csrc/crop.hip (what _augment_rgb is for the colour kernels).  Everything is float32,
# in the order written, one rounding per operation: the device follows it operation for operation and is compared for equality.
_F = np.float32


def _crop_axis(origin, extent, size: int):
    """centres of the `size` output pixels of one axis in source units, u = origin + (o + 0.5) * (extent / size) -> (u, tap index
    floor(u - 0.5), its weight complement a = (u - 0.5) - floor(u - 0.5)), all (size,) arrays"""
    step = _F(extent) / _F(size)
    u = _F(origin) + (np.arange(size, dtype=np.float32) + _F(0.5)) * step
    t = u - _F(0.5)
    f = np.floor(t)
    return u, f.astype(np.int64), t - f


def _resample_rect(src_f32, window, qw: int, qh: int, fill):
    """the bilinear value v, BEFORE rounding to a byte, of the window (x0, y0, w, h) of one float32 image (H, W, 3) mapped onto
    qh x qw output pixels; a tap outside the image is `fill` -> float32 (qh, qw, 3)"""
    h, w, _ = src_f32.shape
    x0, y0, ww, wh = window
    _, xf, ax = _crop_axis(x0, ww, qw)
    _, yf, ay = _crop_axis(y0, wh, qh)

    def tap(yy, xx):
        inside = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
        t = src_f32[np.clip(yy, 0, h - 1)[:, None], np.clip(xx, 0, w - 1)[None, :]]
        return np.where(inside[..., None], t, fill)

    t00, t01, t10, t11 = tap(yf, xf), tap(yf, xf + 1), tap(yf + 1, xf), tap(yf + 1, xf + 1)
    ax3, ay3 = ax[None, :, None], ay[:, None, None]
    top = t00 + (t01 - t00) * ax3
    bot = t10 + (t11 - t10) * ax3
    return top + (bot - top) * ay3


def _nearest_rect(mask_u8, window, qw: int, qh: int, fill_class):
    """the nearest class index of the window (x0, y0, w, h) of one uint8 mask (H, W) mapped onto qh x qw output pixels,
    `fill_class` outside the mask -> uint8 (qh, qw)"""
    h, w = mask_u8.shape
    x0, y0, ww, wh = window
    ux, _, _ = _crop_axis(x0, ww, qw)
    uy, _, _ = _crop_axis(y0, wh, qh)
    xx, yy = np.floor(ux).astype(np.int64), np.floor(uy).astype(np.int64)
    inside = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
    return np.where(inside, mask_u8[np.clip(yy, 0, h - 1)[:, None], np.clip(xx, 0, w - 1)[None, :]], np.uint8(fill_class))


def _to_byte(v):
    return np.floor(v + _F(0.5)).astype(np.uint8)


def _crop_resample_float(images_u8, windows, fill=(0, 0, 0)):
    """the bilinear value v of every output pixel BEFORE rounding to a byte, float32 (B, H, W, 3)"""
    images = np.asarray(images_u8, np.uint8)
    b, h, w, _ = images.shape
    windows = np.asarray(windows, np.float32).reshape(b, 4)
    fill = np.asarray(fill, np.float32).reshape(3)
    out = np.empty((b, h, w, 3), np.float32)
    for n in range(b):
        out[n] = _resample_rect(images[n].astype(np.float32), windows[n], w, h, fill)
    return out


def _crop_resample(images_u8, masks_u8, windows, fill=(0, 0, 0), fill_class=0):
    """(uint8 images (B, H, W, 3) or None, uint8 class indices (B, H, W) or None) seen through one window (x0, y0, w, h) per
    sample: bilinear pixels with `fill` outside the image, byte = floor(v + 0.5); nearest-neighbour class indices with
    `fill_class` outside.  -> (images, masks) of the same shapes"""
    out_img = out_mask = None
    if images_u8 is not None:
        out_img = _to_byte(_crop_resample_float(images_u8, windows, fill))
    if masks_u8 is not None:
        masks = np.asarray(masks_u8, np.uint8)
        b, h, w = masks.shape
        windows = np.asarray(windows, np.float32).reshape(b, 4)
        out_mask = np.empty((b, h, w), np.uint8)
        for n in range(b):
            out_mask[n] = _nearest_rect(masks[n], windows[n], w, h, fill_class)
    return out_img, out_mask


def _rows_through(g, window, rect, height: int, width: int):
    """the ground-truth rows (label, xmin, ymin, xmax, ymax) of one sample that survive the window (x0, y0, w, h) mapped onto the
    rectangle (qx, qy, qw, qh) of an image, in their order: the centre lies in [x0, x0 + w) x [y0, y0 + h) and, after x' = qx +
    (x - x0) (qw / w) clipped to [qx, qx + qw] and y' likewise, the box is at least 1 x 1.  The whole image seen through exactly
    (0, 0, W, H) returns the rows verbatim.  -> (G', 5) float32"""
    g = np.asarray(g, np.float32).reshape(-1, 5)
    x0, y0, ww, wh = (_F(v) for v in window)
    qx, qy, qw, qh = (_F(v) for v in rect)
    W, H = _F(width), _F(height)
    if qw == W and qh == H and x0 == 0 and y0 == 0 and ww == W and wh == H:
        return g.copy()
    kx, ky = qw / ww, qh / wh
    cx, cy = (g[:, 1] + g[:, 3]) * _F(0.5), (g[:, 2] + g[:, 4]) * _F(0.5)
    inside = (x0 <= cx) & (cx < x0 + ww) & (y0 <= cy) & (cy < y0 + wh)
    xmin, xmax = np.clip(qx + (g[:, 1] - x0) * kx, qx, qx + qw), np.clip(qx + (g[:, 3] - x0) * kx, qx, qx + qw)
    ymin, ymax = np.clip(qy + (g[:, 2] - y0) * ky, qy, qy + qh), np.clip(qy + (g[:, 4] - y0) * ky, qy, qy + qh)
    keep = inside & (xmax - xmin >= 1) & (ymax - ymin >= 1)
    return np.stack([g[:, 0], xmin, ymin, xmax, ymax], axis=1).astype(np.float32)[keep]


def _crop_gt(gt_list, windows, height: int, width: int):
    """per sample the ground-truth rows (label, xmin, ymin, xmax, ymax) that survive its window, in their order: the centre lies in
    [x0, x0 + w) x [y0, y0 + h) and, shifted, scaled by (W / w, H / h) and clipped to the image, the box is at least 1 x 1.  A
    window exactly (0, 0, W, H) returns the rows verbatim.  -> list of (G', 5) float32 arrays"""
    windows = np.asarray(windows, np.float32).reshape(len(gt_list), 4)
    return [_rows_through(g, win, (0, 0, width, height), height, width) for g, win in zip(gt_list, windows)]


def random_crop_windows(rng, n: int, height: int, width: int, probability: float = 0.5, scale=(0.5, 2.0), aspect=(0.75, 4 / 3)):
    """n crop windows (x0, y0, w, h), float32 (n, 4), in the manner of the SSD recipe's sampling: with probability 1 - `probability`
    the identity (0, 0, W, H); otherwise s ~ U(scale), a ~ U(aspect), w = s W sqrt(a), h = s H / sqrt(a) (clamped to the C-ABI's
    [1, 16 W] / [1, 16 H]), x0 ~ U(min(0, W - w), max(0, W - w)) and y0 likewise: a window smaller than the image lies inside it
    (zoom-in), a larger one contains it (zoom-out).  No box is looked at: a crop that loses every box is a background sample."""
    n, W, H = int(n), float(width), float(height)
    if not 0.0 <= float(probability) <= 1.0:
        raise ValueError(f"random crop: probability {probability!r} outside [0, 1]")
    (s_lo, s_hi), (a_lo, a_hi) = (float(v) for v in scale), (float(v) for v in aspect)
    if not (0.0 < s_lo <= s_hi and 0.0 < a_lo <= a_hi):
        raise ValueError(f"random crop: scale {scale!r} / aspect {aspect!r} must be positive (low, high) ranges")
    crop = rng.uniform(0.0, 1.0, n) < float(probability)
    s, a = rng.uniform(s_lo, s_hi, n), rng.uniform(a_lo, a_hi, n)
    tx, ty = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    w = np.clip(s * W * np.sqrt(a), 1.0, 16.0 * W).astype(np.float32)
    h = np.clip(s * H / np.sqrt(a), 1.0, 16.0 * H).astype(np.float32)
    # the slack W - w in float32 (so x0 + w stays on the right side of W up to one rounding), the origin a point of [0, slack]
    dx, dy = _F(W) - w, _F(H) - h
    x0, y0 = (tx * dx).astype(np.float32), (ty * dy).astype(np.float32)
    out = np.stack([x0, y0, w, h], axis=1).astype(np.float32)
    out[~crop] = (0.0, 0.0, W, H)
    return out


_aug_rng = np.random.default_rng(1993)
_crop_rng = np.random.default_rng(1993)     # augmentation_random_crop's own stream: the colour draws of _aug_rng are not disturbed


def _split_crop_options(options: dict, what: str = "random crop", sampler_keys=("probability", "scale", "aspect")):
    """a random_crop (or mosaic) option dict -> (the sampler's keywords, the fill (r, g, b, fill_class))"""
    kw = dict(options)
    unknown = set(kw) - set(sampler_keys) - {"fill", "fill_class"}
    if unknown:
        raise ValueError(f"{what}: unknown option(s) {sorted(unknown)}")
    fill, fill_class = kw.pop("fill", (0, 0, 0)), kw.pop("fill_class", 0)
    try:
        fill = tuple(fill)
    except TypeError:
        raise ValueError(f"{what}: fill must be (r, g, b), got {fill!r}") from None
    if len(fill) != 3:
        raise ValueError(f"{what}: fill must be (r, g, b), got {fill!r}")
    return kw, _check_crop_fill(fill + (fill_class,), f"{what}: fill / fill_class")


def augmentation_random_crop(image_batch, targets_batch=None, **options):
    """random zoom-in crops / zoom-out expansions for a CompactBatch: returns (a new CompactBatch sharing its arrays, with one freshly
    drawn window per sample attached, targets_batch), the analogue of augmentation_rgb_channels on a compact batch.  options: the
    keywords of random_crop_windows plus `fill` (r, g, b) and `fill_class`.  The loader applies the windows on the GPU
    (ssdseg_crop_inputs, ssdseg_crop_gt) before the flip and the colour step.  Float (images, targets) batches are refused: their
    anchors are already encoded and cannot be re-cropped."""
    if not isinstance(image_batch, CompactBatch):
        raise ValueError("augmentation_random_crop takes a CompactBatch: a float (images, targets) batch holds encoded anchors that "
                         "cannot be re-cropped")
    cb = image_batch
    kw, fill = _split_crop_options(options)
    windows = random_crop_windows(_crop_rng, len(cb), cb.images.shape[1], cb.images.shape[2], **kw)
    return CompactBatch(cb.images, cb.mask_index, cb.ground_truth, cb.flip, cb.encoder, rgb_draws=cb.rgb_draws, crop_windows=windows,
                        crop_fill=fill, mosaic=cb.mosaic, mosaic_fill=cb.mosaic_fill), targets_batch


# ---- mosaic: the host spec of csrc/mosaic.hip.  The crop generalised: four (source, window) pairs per output sample, each mapped
# onto a quadrant instead of the whole image -- the same axis, tap and row code as above, float32 in the written order.
class Mosaic:
    """How each of b output samples is assembled from four: `index4` (b, 4) int32, the source of tile k as a POSITION WITHIN THE BATCH
    (0..b-1); `split` (b, 2) int32, the split point (px, py) that cuts the sample into the quadrants 0 top-left [0, px) x [0, py),
    1 top-right [px, W) x [0, py), 2 bottom-left [0, px) x [py, H), 3 bottom-right [px, W) x [py, H) (one of zero width or height is
    empty and contributes nothing); `windows` (b, 4, 4) float32, tile k's window (x0, y0, w, h) in its source's pixel units, mapped
    onto quadrant k.  Validated here as far as it can be without the image size; `check(height, width)` does the rest (the batch
    that takes it calls it)."""

    def __init__(self, index4, split, windows):
        try:
            index4, split = np.asarray(index4), np.asarray(split)
            whole = all(a.dtype.kind in "iu" or (a.astype(np.float64) == np.floor(a.astype(np.float64))).all() for a in (index4, split))
            self.index4 = np.ascontiguousarray(index4, np.int32)
            self.split = np.ascontiguousarray(split, np.int32)
            self.windows = np.ascontiguousarray(windows, np.float32)
        except (TypeError, ValueError):
            raise ValueError("mosaic: index4, split and windows must be arrays of numbers") from None
        b = self.index4.shape[0] if self.index4.ndim == 2 else 0
        if b == 0 or self.index4.shape != (b, 4) or self.split.shape != (b, 2) or self.windows.shape != (b, 4, 4):
            raise ValueError(f"mosaic: index4 {self.index4.shape}, split {self.split.shape}, windows {self.windows.shape} must be (b, 4), (b, 2), "
                             "(b, 4, 4)")
        if not whole:
            raise ValueError("mosaic: index4 and split must be whole numbers")
        if self.index4.min() < 0 or self.index4.max() >= b:
            raise ValueError(f"mosaic: index4 names positions within the batch, 0..{b - 1}")
        if self.split.min() < 0:
            raise ValueError("mosaic: split (px, py) must not be negative")
        if not np.isfinite(self.windows).all() or not (self.windows[..., 2:] >= 1).all():
            raise ValueError("mosaic: windows (x0, y0, w, h) must be finite with w >= 1 and h >= 1")
        self._checked = None        # the (height, width) check() has passed for

    @classmethod
    def _trusted(cls, index4, split, windows, height: int, width: int) -> "Mosaic":
        """the sampler's way in: int32 / int32 / float32 arrays of the right shapes that are in range by construction for samples of
        height x width (a batch is built per training step, and the C-ABI validates the lists once more)"""
        self = cls.__new__(cls)
        self.index4, self.split, self.windows, self._checked = index4, split, windows, (height, width)
        return self

    def __len__(self):
        return int(self.index4.shape[0])

    def check(self, height: int, width: int) -> "Mosaic":
        """the ranges the C-ABI takes (include/ssdseg.h) for samples of height x width, the windows of empty quadrants included"""
        if self._checked == (height, width):
            return self
        if (self.split > np.array([width, height], np.int32)).any():
            raise ValueError(f"mosaic: need 0 <= px <= {width} and 0 <= py <= {height}")
        if not _windows_in_range(self.windows, height, width):
            raise ValueError(f"mosaic windows: need 1 <= w <= {16 * width}, 1 <= h <= {16 * height}, |x0| <= {16 * width}, |y0| <= {16 * height}")
        self._checked = (height, width)
        return self

    def quadrants(self, n: int, height: int, width: int):
        """the four quadrants (qx, qy, qw, qh) of sample n"""
        px, py = (int(v) for v in self.split[n])
        return [(0, 0, px, py), (px, 0, width - px, py), (0, py, px, height - py), (px, py, width - px, height - py)]


def _check_mosaic(mosaic, crop_windows, b: int, height: int, width: int):
    """None, or a Mosaic over b samples of height x width, on a batch without crop windows"""
    if mosaic is None:
        return None
    if not isinstance(mosaic, Mosaic):
        raise ValueError(f"mosaic must be None or a datacoder.Mosaic, got {type(mosaic).__name__}")
    if crop_windows is not None:
        raise ValueError("a batch carries crop windows or a mosaic, not both")
    if len(mosaic) != b:
        raise ValueError(f"mosaic over {len(mosaic)} samples for a batch of {b}")
    return mosaic.check(height, width)


def _mosaic_resample(images_u8, masks_u8, mosaic: Mosaic, fill=(0, 0, 0), fill_class=0):
    """(uint8 images (B, H, W, 3) or None, uint8 class indices (B, H, W) or None) assembled by `mosaic`: quadrant k of output sample
    n shows tile k's window of sample index4[n, k] -- the crop's pixels (_resample_rect: taps confined to the source image, not to
    the window) and class indices (_nearest_rect) of that window on qh x qw output pixels.  -> (images, masks) of the same shapes"""
    fill = np.asarray(fill, np.float32).reshape(3)
    images = None if images_u8 is None else np.asarray(images_u8, np.uint8)
    masks = None if masks_u8 is None else np.asarray(masks_u8, np.uint8)
    b, h, w = (images if images is not None else masks).shape[:3]
    mosaic = _check_mosaic(mosaic, None, b, h, w)
    out_img = None if images is None else np.empty((b, h, w, 3), np.uint8)
    out_mask = None if masks is None else np.empty((b, h, w), np.uint8)
    for n in range(b):
        for k, (qx, qy, qw, qh) in enumerate(mosaic.quadrants(n, h, w)):
            if qw <= 0 or qh <= 0:
                continue
            s, win = int(mosaic.index4[n, k]), mosaic.windows[n, k]
            if images is not None:
                out_img[n, qy:qy + qh, qx:qx + qw] = _to_byte(_resample_rect(images[s].astype(np.float32), win, qw, qh, fill))
            if masks is not None:
                out_mask[n, qy:qy + qh, qx:qx + qw] = _nearest_rect(masks[s], win, qw, qh, fill_class)
    return out_img, out_mask


def _mosaic_gt(gt_list, mosaic: Mosaic, height: int, width: int, gmax: int):
    """per output sample the ground-truth rows of its four tiles, in visiting order -- tile 0..3, empty quadrants skipped, each
    source's surviving rows in their order (_rows_through) -- cut after the first `gmax`.  -> list of (G', 5) float32 arrays"""
    mosaic = _check_mosaic(mosaic, None, len(gt_list), height, width)
    out = []
    for n in range(len(gt_list)):
        rows = [_rows_through(gt_list[int(mosaic.index4[n, k])], mosaic.windows[n, k], rect, height, width)
                for k, rect in enumerate(mosaic.quadrants(n, height, width)) if rect[2] > 0 and rect[3] > 0]
        out.append(np.concatenate(rows + [np.zeros((0, 5), np.float32)])[:int(gmax)])
    return out


_MOSAIC_KEYS = ("probability", "center", "scale")
_RIGHT, _LOWER = np.array([False, True, False, True]), np.array([False, False, True, True])      # tiles 1, 3 / tiles 2, 3


def random_mosaic(rng, n: int, height: int, width: int, probability: float = 0.5, center=(0.3, 0.7), scale=(0.5, 1.0)) -> Mosaic:
    """a Mosaic over a batch of n samples: with probability 1 - `probability` a sample is the identity (all four positions its own,
    split (W, H), windows (0, 0, W, H)); otherwise tile 0 is the sample itself and three partners are uniform over the batch's
    positions, the split is (cx W, cy H) rounded with cx, cy ~ U(center), clamped to [1, W - 1] / [1, H - 1], and every tile has a
    zoom s ~ U(scale) and a window of qw / s x qh / s (clamped to the C-ABI's [1, 16 W] / [1, 16 H]) whose origin is drawn as
    random_crop_windows draws it: inside the image when smaller, containing it when larger.  The number of draws depends on n alone."""
    return _random_mosaics(rng, [n], height, width, probability, center, scale)[0]


def _random_mosaics(rng, sizes, height: int, width: int, probability: float = 0.5, center=(0.3, 0.7), scale=(0.5, 1.0)):
    """random_mosaic for consecutive batches of these sizes from ONE draw (an epoch's batches cost one pass of array arithmetic, not
    one per batch); a single size gives random_mosaic's Mosaic.  -> list of Mosaic"""
    sizes = [int(v) for v in sizes]
    n, W, H = sum(sizes), int(width), int(height)
    if not sizes or min(sizes) <= 0 or W < 2 or H < 2:
        raise ValueError(f"mosaic: batches of {sizes} samples of {H}x{W}: need at least one sample of at least 2x2")
    if not 0.0 <= float(probability) <= 1.0:
        raise ValueError(f"mosaic: probability {probability!r} outside [0, 1]")
    try:
        (c_lo, c_hi), (s_lo, s_hi) = (float(v) for v in center), (float(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError(f"mosaic: center {center!r} / scale {scale!r} must be (low, high) ranges") from None
    if not (0.0 <= c_lo <= c_hi <= 1.0 and 0.0 < s_lo <= s_hi < float("inf")):
        raise ValueError(f"mosaic: center {center!r} must be a (low, high) range in [0, 1], scale {scale!r} a positive one")
    # one draw, whatever comes out of it: columns 0 mosaic or identity, 1-2 the split, 3-6 the zooms, 7-10 / 11-14 the origins,
    # 15-17 the partners (a position of the sample's own batch: floor(u b), its batch starting at `first`)
    u = rng.random((n, 18))
    first, count = np.repeat(np.cumsum([0] + sizes[:-1]), sizes)[:, None], np.repeat(sizes, sizes)[:, None]
    partners = np.minimum((u[:, 15:18] * count).astype(np.int32), count - 1)
    mixed = (u[:, 0] < float(probability))[:, None]
    centre = c_lo + (c_hi - c_lo) * u[:, 1:3]
    size = np.array([W, H], np.int32)
    split = np.minimum(np.maximum(np.rint(centre * size), 1), size - 1).astype(np.int32)
    s = s_lo + (s_hi - s_lo) * u[:, 3:7]
    windows = np.empty((n, 4, 4), np.float32)
    windows[..., 2] = np.minimum(np.maximum(np.where(_RIGHT, W - split[:, :1], split[:, :1]) / s, 1.0), 16.0 * W)
    windows[..., 3] = np.minimum(np.maximum(np.where(_LOWER, H - split[:, 1:], split[:, 1:]) / s, 1.0), 16.0 * H)
    # the slack W - w in float32, the origin a point of [0, slack] (as random_crop_windows)
    windows[..., 0] = u[:, 7:11] * (_F(W) - windows[..., 2])
    windows[..., 1] = u[:, 11:15] * (_F(H) - windows[..., 3])
    own = np.arange(n, dtype=np.int32)[:, None] - first
    index4 = np.empty((n, 4), np.int32)
    index4[:, :1], index4[:, 1:] = own, np.where(mixed, partners, own)
    split = np.where(mixed, split, size)
    windows = np.where(mixed[:, :, None], windows, np.array([0, 0, W, H], np.float32))
    split, cuts = np.ascontiguousarray(split, np.int32), np.cumsum([0] + sizes)
    return [Mosaic._trusted(index4[lo:hi], split[lo:hi], windows[lo:hi], H, W) for lo, hi in zip(cuts[:-1], cuts[1:])]


_mosaic_rng = np.random.default_rng(1993)   # augmentation_mosaic's own stream: neither the colour draws nor the crop windows are disturbed


def augmentation_mosaic(image_batch, targets_batch=None, **options):
    """a random mosaic for a CompactBatch: returns (a new CompactBatch sharing its arrays, with a freshly drawn Mosaic over its own
    samples attached, targets_batch), the analogue of augmentation_random_crop.  options: the keywords of random_mosaic plus `fill`
    (r, g, b) and `fill_class`.  The loader assembles the images on the GPU (ssdseg_mosaic_inputs, ssdseg_mosaic_gt) before the flip
    and the colour step.  Float (images, targets) batches are refused: their anchors are already encoded."""
    if not isinstance(image_batch, CompactBatch):
        raise ValueError("augmentation_mosaic takes a CompactBatch: a float (images, targets) batch holds encoded anchors that cannot "
                         "be reassembled")
    cb = image_batch
    kw, fill = _split_crop_options(options, "mosaic", _MOSAIC_KEYS)
    mosaic = random_mosaic(_mosaic_rng, len(cb), cb.images.shape[1], cb.images.shape[2], **kw)
    return CompactBatch(cb.images, cb.mask_index, cb.ground_truth, cb.flip, cb.encoder, rgb_draws=cb.rgb_draws, crop_windows=cb.crop_windows,
                        crop_fill=cb.crop_fill, mosaic=mosaic, mosaic_fill=fill), targets_batch


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
        return CompactBatch(cb.images, cb.mask_index, cb.ground_truth, cb.flip, cb.encoder, rgb_draws=draws, crop_windows=cb.crop_windows,
                            crop_fill=cb.crop_fill, mosaic=cb.mosaic, mosaic_fill=cb.mosaic_fill), targets_batch
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
    draws (`rgb_draws` or None), and optionally one crop window per sample (`crop_windows`, `crop_fill`, as CompactBatch) or a
    mosaic (`mosaic`, `mosaic_fill`, as CompactBatch: its sources are positions within this batch, not pool slots) -- a few host
    bytes; the pixels stay on the device.  `Model.fit` / `train_on_batch` accept it."""

    def __init__(self, dataset: "ResidentDataset", index, flip=None, rgb_draws=None, *, crop_windows=None, crop_fill=None, mosaic=None,
                 mosaic_fill=None):
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
        self.crop_windows = _check_crop_windows(crop_windows, self.index.size, dataset.height, dataset.width)
        self.crop_fill = _check_crop_fill(crop_fill)
        self.mosaic = _check_mosaic(mosaic, self.crop_windows, self.index.size, dataset.height, dataset.width)
        self.mosaic_fill = _check_crop_fill(mosaic_fill, "mosaic_fill")

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
    of samples), filled with `append` / `write` without holding the set on the host.
    `random_crop`: None (the chain above, nothing else drawn), or a dict of random_crop_windows' keywords plus optional `fill` (r, g,
    b) / `fill_class`: every batch then carries one crop window per sample, drawn from the same Generator AFTER the epoch's
    permutation, flips and colour draws, and the device crops before it flips and colours (ssdseg_crop_inputs, ssdseg_crop_gt).
    `mosaic`: None, or a dict of random_mosaic's keywords plus optional `fill` / `fill_class`: every batch then carries a Mosaic over
    its own samples, drawn from the same Generator AFTER the epoch's plan likewise, and the device assembles each image from four
    samples of the batch in the crop's place (ssdseg_mosaic_inputs, ssdseg_mosaic_gt).  Not together with `random_crop`."""

    GMAX = 64       # ground-truth rows per sample, as the compact loader (the encode kernel holds them in LDS)

    def __init__(self, encoder: "DataEncoderDecoder", samples=None, *, capacity: Optional[int] = None, batch_size: int = 16,
                 shuffle: bool = True, rgb_augmentation: bool = False, drop_remainder: bool = False, seed=None, random_crop=None,
                 mosaic=None):
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
        self.random_crop = None
        if random_crop is not None:
            self.random_crop = _split_crop_options(random_crop)
            random_crop_windows(np.random.default_rng(0), 1, self.height, self.width, **self.random_crop[0])      # bad options fail here
        self.mosaic = None
        if mosaic is not None:
            if random_crop is not None:
                raise ValueError("resident dataset: random_crop or mosaic, not both")
            self.mosaic = _split_crop_options(mosaic, "mosaic", _MOSAIC_KEYS)
            random_mosaic(np.random.default_rng(0), 1, self.height, self.width, **self.mosaic[0])                # bad options fail here
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

    def batch(self, index, flip=None, rgb_draws=None, *, crop_windows=None, crop_fill=None, mosaic=None, mosaic_fill=None) -> ResidentBatch:
        """an explicit batch: these samples, seen through these crop windows or assembled by this mosaic, mirrored where flagged, with
        these colour draws"""
        return ResidentBatch(self, index, flip, rgb_draws, crop_windows=crop_windows, crop_fill=crop_fill, mosaic=mosaic, mosaic_fill=mosaic_fill)

    def __iter__(self):
        plan = _epoch_plan(self._rng, self.num_samples, self.batch_size, self.shuffle, bool(self.encoder.augmentation_horizontal_flip),
                           self.rgb_augmentation, self.drop_remainder)
        if self.mosaic is not None:        # drawn after the whole plan, as the windows below; one draw for the epoch's batches
            kw, fill = self.mosaic
            mosaics = _random_mosaics(self._rng, [len(index) for index, _, _ in plan], self.height, self.width, **kw) if plan else []
            return iter([ResidentBatch(self, index, flip, draws, mosaic=mosaic, mosaic_fill=fill)
                         for (index, flip, draws), mosaic in zip(plan, mosaics)])
        if self.random_crop is None:
            return iter([ResidentBatch(self, index, flip, draws) for index, flip, draws in plan])
        kw, fill = self.random_crop        # the windows come after the whole plan: the plan's draws are those of random_crop=None
        return iter([ResidentBatch(self, index, flip, draws, crop_windows=random_crop_windows(self._rng, len(index), self.height, self.width, **kw),
                                   crop_fill=fill) for index, flip, draws in plan])

    def to_compact(self, batch: ResidentBatch) -> CompactBatch:
        """the named samples downloaded into an equal CompactBatch (same windows or mosaic, same flips, same draws): for debugging and
        tests"""
        hw = self.height * self.width
        images = np.stack([self.images.view(int(i) * hw * 3, (self.height, self.width, 3)).download() for i in batch.index])
        masks = np.stack([self.masks.view(int(i) * hw, (self.height, self.width)).download() for i in batch.index])
        cnt = self.cnt.download()
        gts = [self.gt.view(int(i) * self.GMAX * 5, (self.GMAX, 5)).download()[:cnt[i]] for i in batch.index]
        flip = np.zeros(len(batch), np.uint8) if batch.flip is None else batch.flip.copy()
        return CompactBatch(images, masks, gts, flip, self.encoder, rgb_draws=batch.rgb_draws, crop_windows=batch.crop_windows,
                            crop_fill=batch.crop_fill, mosaic=batch.mosaic, mosaic_fill=batch.mosaic_fill)


def read_image(path_file_image: str) -> np.ndarray:
    """PNG -> float32 (H, W, 3) in 0..255 (reference datacoder.py:468-484)."""
    from PIL import Image
    return np.asarray(Image.open(path_file_image).convert("RGB"), np.float32)
