"""The host specifications of the augmentation kernels: csrc/crop.hip (`_crop_resample`, `_crop_gt`), csrc/mosaic.hip
(`_mosaic_resample`, `_mosaic_gt`) and the colour kernel of csrc/inputs.hip (`_augment_rgb`).  The crop and the mosaic are float32
in the order written, one rounding per operation: the device follows them operation for operation and the GPU tests compare for
equality.  Only `datacoder.augmentation_rgb_channels` on float arrays runs any of this outside the tests.  numpy only; `datacoder`
re-exports the names.
"""
import numpy as np

from ._batches import Mosaic, _check_mosaic

# ---- random crop / zoom-out: the host spec of csrc/crop.hip
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


# ---- mosaic: the host spec of csrc/mosaic.hip.  The crop generalised: four (source, window) pairs per output sample, each mapped
# onto a quadrant instead of the whole image -- the same axis, tap and row code as above, float32 in the written order.
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


# ---- colour: the host spec of ssdseg_rgb_augment (compared within a tolerance: `mean` is a reduction)
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
