"""The host side of the random crop / zoom-out augmentation (datacoder._crop_resample, _crop_gt, random_crop_windows, the
`crop_windows` / `crop_fill` keywords of CompactBatch / ResidentBatch and ResidentDataset(random_crop=...)): the NumPy float32 spec
the device kernels of csrc/crop.hip are compared with byte for byte (tests/test_gpu_random_crop.py), checked here against an
independent implementation (torch.nn.functional.grid_sample in float64), hand-worked boxes and the parent's RNG stream.  No GPU."""
import numpy as np
import pytest

SHAPES = [(24, 36), (15, 22)]
FILLS = [(0, 0, 0), (124, 116, 104)]


def crop_windows(H, W):
    """the named windows (x0, y0, w, h) of the parity tests, in this order"""
    return {
        "identity": (0, 0, W, H),
        "zoom-in, fractional origin": (3.25, 2.5, W / 2, H / 2),
        "zoom-out": (-W / 2, -H / 4, 2 * W, 1.5 * H),
        "half outside": (0.6 * W, -2, 0.7 * W, 0.9 * H),
        "integer-aligned": (4, 3, 8, 6),
        "extreme magnification": (5.3, 4.1, 1.5, 1.25),
        "anisotropic": (1, 2, 0.37 * W, 0.81 * H),
    }


def _grid_sample_f64(image_u8, window, fill):
    """the independent implementation: grid_sample (bilinear, zeros outside, align_corners=False) of image - fill, + fill, float64"""
    import torch
    H, W, _ = image_u8.shape
    x0, y0, w, h = (float(np.float32(v)) for v in window)
    fill = torch.tensor(fill, dtype=torch.float64)
    src = (torch.from_numpy(image_u8.astype(np.float64)) - fill).permute(2, 0, 1)[None]
    ox, oy = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)
    gx = 2 * ((ox + 0.5) * w / W + x0) / W - 1
    gy = 2 * ((oy + 0.5) * h / H + y0) / H - 1
    grid = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W)], dim=-1)[None]
    out = torch.nn.functional.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    return (out[0].permute(1, 2, 0) + fill).numpy()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_crop_resample_against_grid_sample(rng, H, W, fill):
    """float32 spec vs float64 grid_sample.  2e-3 on the value before rounding: a prototype of the spec was within 6.5e-4 (float32
    against float64 at magnitudes <= 255), so about 3x that; the bytes differ by at most 1, and only at rounding ties"""
    from ssdseglib import datacoder as D
    image = rng.integers(0, 256, (1, H, W, 3)).astype(np.uint8)
    for name, window in crop_windows(H, W).items():
        win = np.array([window], np.float32)
        v = D._crop_resample_float(image, win, fill)
        want = _grid_sample_f64(image[0], win[0], fill)
        err = np.abs(v[0].astype(np.float64) - want).max()
        print(f"{H}x{W} fill {fill} {name}: max |float32 spec - float64 grid_sample| = {err:.3g}")
        assert v.dtype == np.float32 and err <= 2e-3, (name, err)
        got, _ = D._crop_resample(image, None, win, fill, 0)
        assert got.dtype == np.uint8 and got.shape == image.shape
        assert np.abs(got[0].astype(np.int64) - np.floor(want + 0.5).astype(np.int64)).max() <= 1, name
        if name == "identity":
            assert got.tobytes() == image.tobytes()


@pytest.mark.parametrize("H,W", SHAPES)
def test_crop_mask_is_nearest_neighbour(rng, H, W):
    """against a plain integer-indexing restatement of the issue's formula, pixel by pixel: exact"""
    from ssdseglib import datacoder as D
    f = np.float32
    mask = rng.integers(0, 6, (1, H, W)).astype(np.uint8)
    for name, window in crop_windows(H, W).items():
        for fill_class in (0, 5):
            x0, y0, w, h = (f(v) for v in window)
            sx, sy = w / f(W), h / f(H)
            want = np.empty((H, W), np.uint8)
            for oy in range(H):
                yy = int(np.floor(y0 + (f(oy) + f(0.5)) * sy))
                for ox in range(W):
                    xx = int(np.floor(x0 + (f(ox) + f(0.5)) * sx))
                    want[oy, ox] = mask[0, yy, xx] if 0 <= yy < H and 0 <= xx < W else fill_class
            _, got = D._crop_resample(None, mask, np.array([window], np.float32), (0, 0, 0), fill_class)
            assert got.dtype == np.uint8
            np.testing.assert_array_equal(got[0], want, err_msg=name)
            if name == "identity":
                assert got.tobytes() == mask.tobytes()


# ---- ground-truth rows, worked by hand: a 100 x 100 image seen through (x0, y0, w, h) = (20, 10, 50, 40), so kx = 2, ky = 2.5
WINDOW = (20, 10, 50, 40)
GT_CASES = [
    # (row, the row after the crop or None when it is dropped)
    ((1, 10, 20, 30, 40), (1, 0, 25, 20, 75)),               # centre x = 20: exactly on the left edge, kept; clipped on the left
    ((2, 60, 20, 80, 40), None),                             # centre x = 70: exactly on the right edge, dropped
    ((3, 15, 0, 45, 30), (3, 0, 0, 50, 50)),                 # clipped on two sides: left and top
    ((1, 19.75, 20, 20.375, 40), None),                      # 1.25 px wide unclipped, 0.75 px after the clip at 0: dropped
    ((2, 30, 12, 40, 12.25), None),                          # 0.625 px high: dropped
    ((3, 30, 20, 40, 30), (3, 20, 25, 40, 50)),              # inside
    ((1, 40, 10, 90, 50), (1, 40, 0, 100, 100)),             # centre (65, 30): kept, clipped right and bottom; centre y = 30
    ((2, 30, 40, 40, 60), None),                             # centre y = 50: exactly on the bottom edge, dropped
    ((3, 30, 0, 40, 20), (3, 20, 0, 40, 25)),                # centre y = 10: exactly on the top edge, kept
]


def test_crop_gt_hand_worked():
    from ssdseglib import datacoder as D
    rows = np.array([r for r, _ in GT_CASES], np.float32)
    want = np.array([w for _, w in GT_CASES if w is not None], np.float32)
    outside = np.array([[1, 0, 0, 10, 10], [2, 80, 60, 99, 99]], np.float32)
    sticks_out = np.array([[2, -5, -5, 120, 130], [1, 19.75, 20, 20.375, 40]], np.float32)
    got = D._crop_gt([rows, outside, np.zeros((0, 5), np.float32), sticks_out, rows[::-1]],
                     [WINDOW, WINDOW, WINDOW, (0, 0, 100, 100), WINDOW], 100, 100)
    assert all(g.dtype == np.float32 and g.ndim == 2 and g.shape[1] == 5 for g in got)
    np.testing.assert_array_equal(got[0], want)               # kept rows compacted in their order, values exact
    assert got[1].shape == (0, 5) and got[2].shape == (0, 5)  # every row dropped / none to begin with: count 0
    np.testing.assert_array_equal(got[3], sticks_out)         # identity: verbatim, no centre test, no clip
    np.testing.assert_array_equal(got[4], want[::-1])         # the order follows the source
    # the identity is the exact window only: one ulp off and the rows go through the test and the clip
    near = D._crop_gt([sticks_out], [(0, 0, 100, np.nextafter(np.float32(100), np.float32(0)))], 100, 100)[0]
    assert near.shape == (1, 5) and near[0, 1] == 0 and near[0, 3] == 100


def test_sampler():
    from ssdseglib import datacoder as D
    H, W, n = 96, 128, 4000
    a = D.random_crop_windows(np.random.default_rng(5), n, H, W)
    b = D.random_crop_windows(np.random.default_rng(5), n, H, W)
    assert a.dtype == np.float32 and a.shape == (n, 4) and a.tobytes() == b.tobytes()
    assert a.tobytes() != D.random_crop_windows(np.random.default_rng(6), n, H, W).tobytes()
    identity = (a == np.array([0, 0, W, H], np.float32)).all(axis=1)
    assert abs(identity.mean() - 0.5) < 0.05                  # 4000 draws at p = 0.5: sigma = 0.008
    share = (D.random_crop_windows(np.random.default_rng(5), n, H, W, probability=0.9) == np.array([0, 0, W, H], np.float32)).all(axis=1).mean()
    assert abs(share - 0.1) < 0.03
    assert (D.random_crop_windows(np.random.default_rng(5), 50, H, W, probability=0.0) == np.array([0, 0, W, H], np.float32)).all()
    for win, (Hh, Ww) in ((a[~identity], (H, W)), (D.random_crop_windows(np.random.default_rng(7), n, 15, 22, 1.0, (0.02, 40.0), (0.1, 10.0)), (15, 22))):
        x0, y0, w, h = (win[:, k].astype(np.float64) for k in range(4))
        # the C-ABI's ranges
        assert np.isfinite(win).all() and (w >= 1).all() and (w <= 16 * Ww).all() and (h >= 1).all() and (h <= 16 * Hh).all()
        assert (np.abs(x0) <= 16 * Ww).all() and (np.abs(y0) <= 16 * Hh).all()
        # inside / containing, up to the float32 rounding of x0 + w at magnitudes <= 16 W (one ulp there is 16 W * 2^-23)
        tol = 4 * 16 * max(Hh, Ww) * 2.0 ** -23
        for o, e, size in ((x0, w, Ww), (y0, h, Hh)):
            small = e <= size
            assert (o[small] >= 0).all() and (o[small] + e[small] <= size + tol).all()
            assert (o[~small] <= 0).all() and (o[~small] + e[~small] >= size - tol).all()
    scale = a[~identity][:, 2] * a[~identity][:, 3] / (H * W)  # w h = s^2 W H
    assert 0.25 - 1e-3 <= scale.min() and scale.max() <= 4.0 + 1e-3 and scale.min() < 0.5 and scale.max() > 3.0
    with pytest.raises(ValueError):
        D.random_crop_windows(np.random.default_rng(5), 4, H, W, probability=1.5)
    with pytest.raises(ValueError):
        D.random_crop_windows(np.random.default_rng(5), 4, H, W, scale=(0.0, 1.0))


N, B = 11, 4


def _dataset(**kw):
    """a dataset of N samples that never touches a device (as tests/test_cpu_resident_dataset.py): only the sample count is set"""
    from ssdseglib import datacoder as D
    z = np.zeros(3, np.float32)
    enc = D.DataEncoderDecoder(4, (6, 8), xmin_boxes_default=z, ymin_boxes_default=z, xmax_boxes_default=z + 1, ymax_boxes_default=z + 1,
                               augmentation_horizontal_flip=True)
    ds = D.ResidentDataset(enc, capacity=N, batch_size=B, **kw)
    ds.num_samples = N
    return ds


def test_rng_stream_without_the_option_is_the_epoch_plan():
    """random_crop=None: two epochs are the index / flip / colour-draw lists of _epoch_plan on an identically seeded Generator (what
    the dataset did before the option existed).  With the option, the windows are drawn after the epoch's plan: the first epoch's
    plan is still that one."""
    from ssdseglib import datacoder as D
    ds = _dataset(seed=21, rgb_augmentation=True, random_crop=None)
    twin = np.random.default_rng(21)
    for _ in range(2):
        plan = D._epoch_plan(twin, N, B, True, True, True, False)
        batches = list(ds)
        assert len(batches) == len(plan) == 3
        for rb, (index, flip, draws) in zip(batches, plan):
            assert np.array_equal(rb.index, index) and np.array_equal(rb.flip, flip) and rb.rgb_draws == draws
            assert rb.crop_windows is None and rb.crop_fill is None
    cropped = _dataset(seed=21, rgb_augmentation=True, random_crop=dict(probability=0.7, scale=(0.5, 1.5), fill=(124, 116, 104), fill_class=3))
    plan = D._epoch_plan(np.random.default_rng(21), N, B, True, True, True, False)
    batches = list(cropped)
    for rb, (index, flip, draws) in zip(batches, plan):
        assert np.array_equal(rb.index, index) and np.array_equal(rb.flip, flip) and rb.rgb_draws == draws
        assert rb.crop_windows.dtype == np.float32 and rb.crop_windows.shape == (len(rb), 4) and rb.crop_fill == (124, 116, 104, 3)
    again = list(_dataset(seed=21, rgb_augmentation=True, random_crop=dict(probability=0.7, scale=(0.5, 1.5))))
    assert all(np.array_equal(a.crop_windows, b.crop_windows) for a, b in zip(again, batches)) and again[0].crop_fill == (0, 0, 0, 0)
    assert not np.array_equal(np.concatenate([rb.crop_windows for rb in cropped]), np.concatenate([rb.crop_windows for rb in batches]))
    with pytest.raises(ValueError):
        _dataset(random_crop=dict(zoom=2))
    with pytest.raises(ValueError):
        _dataset(random_crop=dict(fill=(0, 0, 256)))


def _compact(b=2, H=6, W=8, **kw):
    from ssdseglib import datacoder as D
    return D.CompactBatch(np.zeros((b, H, W, 3), np.uint8), np.zeros((b, H, W), np.uint8), [np.zeros((0, 5), np.float32)] * b, None, None, **kw)


def test_crop_windows_are_validated():
    from ssdseglib import datacoder as D
    good = [(0, 0, 8, 6), (1.5, -2, 4, 3)]
    cb = _compact(crop_windows=good, crop_fill=(1, 2, 3, 1))
    assert cb.crop_windows.dtype == np.float32 and cb.crop_windows.shape == (2, 4) and cb.crop_fill == (1, 2, 3, 1)
    assert _compact().crop_windows is None and _compact().crop_fill is None
    ds = _dataset(seed=1)
    rb = ds.batch([3, 0], [1, 0], None, crop_windows=good, crop_fill=(9, 9, 9, 0))
    assert rb.crop_windows.shape == (2, 4) and rb.crop_fill == (9, 9, 9, 0)
    assert ds.batch([3, 0], [1, 0], (0, 1, 1, 0)).crop_windows is None          # the positional form of before
    bad_windows = [good[:1], [(0, 0, 8)] * 2, np.zeros((2, 2, 4)), [(0, 0, 8, 6), (0, 0, float("nan"), 6)], [(0, 0, 8, 6), (float("inf"), 0, 8, 6)],
                   [(0, 0, 0.5, 6)] * 2, [(0, 0, 8, 16 * 6 + 1)] * 2, [(17 * 8, 0, 8, 6)] * 2, "ab"]
    for bad in bad_windows:
        with pytest.raises(ValueError):
            _compact(crop_windows=bad)
        with pytest.raises(ValueError):
            ds.batch([3, 0], crop_windows=bad)
    for bad in [(0, 0, 0), (0, 0, 0, 256), (0, -1, 0, 0), (0.5, 0, 0, 0), "abcd"]:
        with pytest.raises(ValueError):
            _compact(crop_windows=good, crop_fill=bad)
    with pytest.raises(TypeError):
        D.CompactBatch(np.zeros((2, 6, 8, 3), np.uint8), np.zeros((2, 6, 8), np.uint8), [np.zeros((0, 5))] * 2, None, None, None, good)   # keyword-only


def test_augmentation_random_crop():
    from ssdseglib import datacoder as D
    cb = _compact(b=3, rgb_draws=(0.01, 1.0, 1.0, 0.0))
    targets = object()
    out, t = D.augmentation_random_crop(cb, targets, probability=1.0, fill=(1, 2, 3), fill_class=2)
    assert t is targets and isinstance(out, D.CompactBatch) and out is not cb and cb.crop_windows is None
    assert out.images is cb.images and out.rgb_draws == cb.rgb_draws
    assert out.crop_windows.shape == (3, 4) and out.crop_fill == (1, 2, 3, 2)
    assert not (out.crop_windows == np.array([0, 0, 8, 6], np.float32)).all(axis=1).any()
    state = D._aug_rng.bit_generator.state
    coloured, _ = D.augmentation_rgb_channels(out, None)              # the colour step on top keeps the windows
    D._aug_rng.bit_generator.state = state                            # (and this test leaves the colour stream where it was)
    assert np.array_equal(coloured.crop_windows, out.crop_windows) and coloured.crop_fill == out.crop_fill and coloured.rgb_draws != cb.rgb_draws
    other, _ = D.augmentation_random_crop(cb)
    assert not np.array_equal(other.crop_windows, D.augmentation_random_crop(cb, probability=1.0)[0].crop_windows)      # fresh draws
    with pytest.raises(ValueError, match="CompactBatch"):
        D.augmentation_random_crop(np.zeros((2, 6, 8, 3), np.float32), {"output-boxes": np.zeros((2, 4, 4), np.float32)})
