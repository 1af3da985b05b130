"""What the input pipeline draws, from a numpy Generator handed in: crop windows, mosaics and one epoch's plan of a resident
dataset, plus the option dicts that configure them.  No device, no stream of its own: `datacoder`'s augmentation_* callables and
`_resident.ResidentDataset` own the generators.  `datacoder` re-exports the public names.
"""
import numpy as np

from ._batches import Mosaic, _check_crop_fill

_F = np.float32


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


# ---- one epoch of a resident dataset: NB03#cell8's shuffle / map(read_and_encode) / batch / map(augmentation) chain
_RGB_RANGES = ((-0.05, 0.05), (0.95, 1.05), (0.90, 1.10), (-0.10, 0.10))     # the ranges of datacoder._draw_rgb (reference datacoder.py:452-461)


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
