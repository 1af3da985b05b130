"""The batch containers of the compact hand-over: `CompactBatch` (what the files hold, on the host), `ResidentBatch` (a list of
samples of a `_resident.ResidentDataset`) and the `Mosaic` a batch may carry.  Both batches are an `_AugmentedBatch`: the five
augmentation fields (`rgb_draws`, `crop_windows`, `crop_fill`, `mosaic`, `mosaic_fill`) are validated, copied, paired into the
geometric step and asked "is this batch plain" in that one class.  Host only: numpy, no device.  `datacoder` re-exports the public
names.
"""
import numpy as np

GMAX = 64       # ground-truth rows per sample in every padded (b, GMAX, 5) buffer: the encode kernel holds them in LDS (boxes.hip)


def pad_ground_truth(ground_truth, gmax: int):
    """per-image (k_i, 5) rows, k_i <= gmax (the caller's check, and its error) -> gt (b, gmax, 5) float32, zero-padded, and cnt (b,)
    int32"""
    gt = np.zeros((len(ground_truth), gmax, 5), np.float32)
    cnt = np.zeros(len(ground_truth), np.int32)
    for i, g in enumerate(ground_truth):
        g = np.asarray(g, np.float32).reshape(-1, 5)
        gt[i, :g.shape[0]] = g
        cnt[i] = g.shape[0]
    return gt, cnt


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


class _AugmentedBatch:
    """What a CompactBatch and a ResidentBatch carry besides their samples, all applied on the device when the batch is expanded:

      * `flip`: uint8 flags, one per sample, or None;
      * `rgb_draws`: (hue_delta, saturation_factor, contrast_factor, brightness_delta) of augmentation_rgb_channels
        (ssdseg_rgb_augment); None: the pixels go in as they are;
      * `crop_windows`, `crop_fill`: one crop window (x0, y0, w, h) per sample and (r, g, b, fill_class) for what lies outside the
        image (ssdseg_crop_inputs / ssdseg_crop_gt), BEFORE the flip and the colour step; None: no crop;
      * `mosaic`, `mosaic_fill`: a `Mosaic` -- four (source position within this batch, window) pairs per sample around a split point
        -- and its fill (ssdseg_mosaic_inputs / ssdseg_mosaic_gt), in the crop's place; None: no mosaic.  Not both.

    The subclass sets `flip` and its own fields, then calls `_set_augment`; `_rebuild(**five)` is its constructor on its own fields."""

    AUGMENT = ("rgb_draws", "crop_windows", "crop_fill", "mosaic", "mosaic_fill")

    def _set_augment(self, b: int, height: int, width: int, rgb_draws, crop_windows, crop_fill, mosaic, mosaic_fill) -> None:
        self.rgb_draws = _check_rgb_draws(rgb_draws)
        self.crop_windows = _check_crop_windows(crop_windows, b, height, width)
        self.crop_fill = _check_crop_fill(crop_fill)
        self.mosaic = _check_mosaic(mosaic, self.crop_windows, b, height, width)
        self.mosaic_fill = _check_crop_fill(mosaic_fill, "mosaic_fill")

    def augment(self) -> dict:
        """the five fields as constructor keywords (of either kind of batch)"""
        return {name: getattr(self, name) for name in self.AUGMENT}

    def replace(self, **fields):
        """a batch of the same samples, sharing their arrays, with these of the five fields replaced (validated anew; any other
        keyword is the constructor's TypeError)"""
        return self._rebuild(**{**self.augment(), **fields})

    def geometric(self):
        """the geometric step in front of the flip and the colour step, with ITS fill: None, ("crop", windows, crop_fill) or ("mosaic",
        mosaic, mosaic_fill); the kind names the entry pair ssdseg_<kind>_inputs / ssdseg_<kind>_gt"""
        if self.mosaic is not None:
            return "mosaic", self.mosaic, self.mosaic_fill
        if self.crop_windows is not None:
            return "crop", self.crop_windows, self.crop_fill
        return None

    def augmented_by(self):
        """which of "rgb_draws", "crop_windows", "mosaic", "flip" change what the files hold, in that order; empty: a plain batch"""
        carried = [name for name in ("rgb_draws", "crop_windows", "mosaic") if getattr(self, name) is not None]
        return tuple(carried + ["flip"] * bool(self.flip is not None and np.any(self.flip)))


class CompactBatch(_AugmentedBatch):
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

    def __init__(self, images_u8, mask_index_u8, ground_truth, flip, encoder, rgb_draws=None, *, crop_windows=None, crop_fill=None,
                 mosaic=None, mosaic_fill=None):
        self.images = np.ascontiguousarray(images_u8, np.uint8)
        self.mask_index = np.ascontiguousarray(mask_index_u8, np.uint8)
        if self.images.ndim != 4 or self.images.shape[-1] != 3 or self.mask_index.shape != self.images.shape[:3]:
            raise ValueError(f"compact batch: images {self.images.shape} must be (B, H, W, 3) and masks {self.mask_index.shape} (B, H, W)")
        self.ground_truth = [np.asarray(g, np.float32).reshape(-1, 5) for g in ground_truth]
        if len(self.ground_truth) != self.images.shape[0]:
            raise ValueError("compact batch: one ground-truth array per image")
        self.flip = None if flip is None else np.ascontiguousarray(flip, np.uint8).reshape(self.images.shape[0])
        self.encoder = encoder
        self._set_augment(*self.images.shape[:3], rgb_draws, crop_windows, crop_fill, mosaic, mosaic_fill)

    def _rebuild(self, **augment) -> "CompactBatch":
        return CompactBatch(self.images, self.mask_index, self.ground_truth, self.flip, self.encoder, **augment)

    def __len__(self):
        return self.images.shape[0]


class ResidentBatch(_AugmentedBatch):
    """A batch of a ResidentDataset: which samples (`index`, int32), which of them mirrored (`flip`, uint8 or None) and the colour
    draws (`rgb_draws` or None), and optionally one crop window per sample (`crop_windows`, `crop_fill`, as CompactBatch) or a
    mosaic (`mosaic`, `mosaic_fill`, as CompactBatch: its sources are positions within this batch, not pool slots) -- a few host
    bytes; the pixels stay on the device.  `Model.fit` / `train_on_batch` accept it."""

    def __init__(self, dataset, index, flip=None, rgb_draws=None, *, crop_windows=None, crop_fill=None, mosaic=None, mosaic_fill=None):
        self.dataset = dataset
        self.index = np.ascontiguousarray(index, np.int32).reshape(-1)
        if self.index.size == 0:
            raise ValueError("resident batch: no samples")
        if self.index.min() < 0 or self.index.max() >= dataset.num_samples:
            raise IndexError(f"resident batch: sample index outside [0, {dataset.num_samples})")
        self.flip = None if flip is None else np.ascontiguousarray(flip, np.uint8).reshape(-1)
        if self.flip is not None and self.flip.size != self.index.size:
            raise ValueError("resident batch: one flip flag per sample")
        self._set_augment(self.index.size, dataset.height, dataset.width, rgb_draws, crop_windows, crop_fill, mosaic, mosaic_fill)

    def _rebuild(self, **augment) -> "ResidentBatch":
        return ResidentBatch(self.dataset, self.index, self.flip, **augment)

    @property
    def encoder(self):
        return self.dataset.encoder

    def __len__(self):
        return int(self.index.size)
