"""The host side of the mosaic augmentation (datacoder.Mosaic, _mosaic_resample, _mosaic_gt, random_mosaic, the `mosaic` /
`mosaic_fill` keywords of CompactBatch / ResidentBatch and ResidentDataset(mosaic=...)): the NumPy float32 spec the device kernels
of csrc/mosaic.hip are compared with byte for byte (tests/test_gpu_mosaic.py), pinned here independently of any kernel: unit-scale
windows are plain pastes of source rectangles, a single-tile mosaic is the crop, hand-worked boxes, the sampler's ranges and the
dataset's RNG stream.  No GPU."""
import numpy as np
import pytest

from tests.test_cpu_random_crop import GT_CASES, WINDOW, N, B, _compact, _dataset, crop_windows

H, W = 24, 36
FILL, FILL_CLASS = (124, 116, 104), 3


def _sources(rng, n=4, h=H, w=W):
    return rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8), rng.integers(0, 6, (n, h, w)).astype(np.uint8)


def unit_scale_mosaic(px, py, h=H, w=W, origins=((3, 2), (-4, 5), (7, -3), (20, 15))):
    """all four samples of a batch of 4 cut at (px, py), tile k from source (n + k) % 4 at integer origin origins[k] with w = qw, h = qh
    (a window of an empty quadrant is any valid one)"""
    from ssdseglib import datacoder as D
    index4 = np.array([[(n + k) % 4 for k in range(4)] for n in range(4)], np.int32)
    split = np.tile(np.array([px, py], np.int32), (4, 1))
    quads = [(px, py), (w - px, py), (px, h - py), (w - px, h - py)]
    windows = np.array([[(x0, y0, max(qw, 1), max(qh, 1)) for (x0, y0), (qw, qh) in zip(origins, quads)]] * 4, np.float32)
    return D.Mosaic(index4, split, windows)


@pytest.mark.parametrize("px,py", [(W, H), (0, 0), (1, 1), (W - 1, H - 1), (13, 10)], ids=["WxH", "0x0", "1x1", "W-1xH-1", "13x10"])
def test_unit_scale_windows_paste_source_rectangles(rng, px, py):
    """integer x0, y0 and w = qw, h = qh: out[y, x] == src_k[y0 + y - qy, x0 + x - qx] (fill outside the source), and the rows are
    shifted by integers"""
    from ssdseglib import datacoder as D
    assert 13 % 4 != 0
    img, idx = _sources(rng)
    m = unit_scale_mosaic(px, py)
    got_img, got_idx = D._mosaic_resample(img, idx, m, FILL, FILL_CLASS)
    assert got_img.dtype == np.uint8 and got_idx.dtype == np.uint8 and got_img.shape == img.shape and got_idx.shape == idx.shape
    want_img, want_idx = np.empty_like(img), np.empty_like(idx)
    for n in range(4):
        for y in range(H):
            for x in range(W):
                k = (1 if x >= px else 0) + (2 if y >= py else 0)
                qx, qy = (px if k & 1 else 0), (py if k & 2 else 0)
                x0, y0 = (int(v) for v in m.windows[n, k, :2])
                sx, sy, s = x0 + x - qx, y0 + y - qy, m.index4[n, k]
                inside = 0 <= sx < W and 0 <= sy < H
                want_img[n, y, x] = img[s, sy, sx] if inside else FILL
                want_idx[n, y, x] = idx[s, sy, sx] if inside else FILL_CLASS
    np.testing.assert_array_equal(got_img, want_img)
    np.testing.assert_array_equal(got_idx, want_idx)
    # rows: a 2 x 2 box at the corner of every window, in every source; at unit scale a kept row moves by (qx - x0, qy - y0),
    # integers, and is clipped to its quadrant -- restated here in plain Python numbers (all values are small integers: exact)
    gts = [np.array([(k + 1, x0 + 1, y0 + 1, x0 + 3, y0 + 3) for k, (x0, y0) in enumerate(m.windows[0, :, :2].tolist())], np.float32)] * 4
    rows = D._mosaic_gt(gts, m, H, W, 64)
    for n in range(4):
        want = []
        for k, (qx, qy, qw, qh) in enumerate(m.quadrants(n, H, W)):
            if qw <= 0 or qh <= 0:
                continue
            x0, y0 = m.windows[n, k, :2].tolist()
            for label, xmin, ymin, xmax, ymax in gts[m.index4[n, k]].tolist():
                if not (x0 <= (xmin + xmax) / 2 < x0 + qw and y0 <= (ymin + ymax) / 2 < y0 + qh):
                    continue
                box = [min(max(qx + v - x0, qx), qx + qw) for v in (xmin, xmax)] + [min(max(qy + v - y0, qy), qy + qh) for v in (ymin, ymax)]
                if box[1] - box[0] >= 1 and box[3] - box[2] >= 1:
                    want.append((label, box[0], box[2], box[1], box[3]))
        np.testing.assert_array_equal(rows[n], np.array(want, np.float32).reshape(-1, 5))
    if (px, py) == (13, 10):
        assert [len(r) for r in rows] == [4] * 4 and rows[0][:, 0].tolist() == [1, 2, 3, 4]


@pytest.mark.parametrize("h,w", [(24, 36), (15, 22)])
def test_single_tile_mosaic_is_the_crop(rng, h, w):
    from ssdseglib import datacoder as D
    names = list(crop_windows(h, w))
    win = np.array(list(crop_windows(h, w).values()), np.float32)
    b = len(win)
    img, idx = _sources(rng, b, h, w)
    gts = [np.array([r for r, _ in GT_CASES], np.float32) * np.array([1, w / 100, h / 100, w / 100, h / 100], np.float32) for _ in range(b)]
    order = np.array([(3 * n + 1) % b for n in range(b)], np.int32)
    windows = np.tile(np.array([1, 1, 2, 2], np.float32), (b, 4, 1))
    windows[:, 0] = win
    m = D.Mosaic(np.stack([order, order[::-1], order, order], axis=1), np.tile(np.array([w, h], np.int32), (b, 1)), windows)
    got_img, got_idx = D._mosaic_resample(img, idx, m, FILL, FILL_CLASS)
    want_img, want_idx = D._crop_resample(img[order], idx[order], win, FILL, FILL_CLASS)
    np.testing.assert_array_equal(got_img, want_img)
    np.testing.assert_array_equal(got_idx, want_idx)
    rows, want = D._mosaic_gt(gts, m, h, w, 64), D._crop_gt([gts[s] for s in order], win, h, w)
    assert any(len(r) for r in want)
    for name, a, c in zip(names, rows, want):
        np.testing.assert_array_equal(a, c, err_msg=name)
    # image only / mask only
    assert D._mosaic_resample(img, None, m, FILL, FILL_CLASS)[1] is None and D._mosaic_resample(None, idx, m, FILL, FILL_CLASS)[0] is None
    np.testing.assert_array_equal(D._mosaic_resample(None, idx, m, FILL, FILL_CLASS)[1], want_idx)


def identity_mosaic(b, h, w):
    from ssdseglib import datacoder as D
    own = np.arange(b, dtype=np.int32)
    return D.Mosaic(np.tile(own[:, None], (1, 4)), np.tile(np.array([w, h], np.int32), (b, 1)), np.tile(np.array([0, 0, w, h], np.float32), (b, 4, 1)))


def test_identity_returns_bytes_and_rows_verbatim(rng):
    from ssdseglib import datacoder as D
    img, idx = _sources(rng)
    gts = [np.array([[2, -5, -5, 120, 130], [1, 19.75, 20, 20.375, 40]], np.float32), np.zeros((0, 5), np.float32),
           np.array([[3, 1, 1, 1.25, 1.25]], np.float32), np.array([r for r, _ in GT_CASES], np.float32)]
    m = identity_mosaic(4, H, W)
    got_img, got_idx = D._mosaic_resample(img, idx, m, FILL, FILL_CLASS)
    assert got_img.tobytes() == img.tobytes() and got_idx.tobytes() == idx.tobytes()
    for a, c in zip(D._mosaic_gt(gts, m, H, W, 64), gts):
        assert a.dtype == np.float32 and a.tobytes() == c.tobytes()          # sticking out of the image, thinner than 1 px: verbatim
    # the whole image in another quadrant (split (0, 0): tile 3) is verbatim too
    m3 = D.Mosaic(m.index4, np.zeros((4, 2), np.int32), m.windows)
    assert D._mosaic_resample(img, idx, m3, FILL, FILL_CLASS)[0].tobytes() == img.tobytes()
    assert D._mosaic_gt(gts, m3, H, W, 64)[0].tobytes() == gts[0].tobytes()


# ---- ground truth, worked by hand on a 100 x 100 image cut at (40, 60): quadrants 40x60, 60x60, 40x40, 60x40
def test_mosaic_gt_hand_worked():
    from ssdseglib import datacoder as D
    h = w = 100
    src = [
        np.array([(1, 10, 10, 30, 30), (2, 30, 10, 50, 30), (3, 0, 0, 9, 9)], np.float32),       # tile 0, window (0, 0, 40, 60): unit scale
        np.array([(1, 20, 0, 50, 40), (2, 0, 10, 40, 30), (3, 45, 5, 45.5, 35), (4, 30, 20, 40, 40)], np.float32),   # tile 1, window (20, 0, 30, 30): x2
        np.array([(4, 50, 50, 70, 70)], np.float32),                                             # tile 2, window (0, 0, 100, 100): x0.4
        np.array([(5, 10, 10, 12, 50)], np.float32),                                             # tile 3, window (0, 0, 120, 80): x0.5
    ]
    m = D.Mosaic([[0, 1, 2, 3]] + [[0, 0, 0, 0]] * 3, [[40, 60]] + [[100, 100]] * 3,
                 [[(0, 0, 40, 60), (20, 0, 30, 30), (0, 0, 100, 100), (0, 0, 120, 80)]] + [[(0, 0, 100, 100)] * 4] * 3)
    got = D._mosaic_gt(src, m, h, w, 64)[0]
    want = np.array([
        (1, 10, 10, 30, 30),          # tile 0: unit scale, inside.  Its row 2 has centre x = 40, exactly on the right edge: dropped
        (3, 0, 0, 9, 9),
        (1, 40, 0, 100, 60),          # tile 1: centre (35, 20); x 40 + (20 - 20) 2 = 40, 40 + (50 - 20) 2 = 100; y 0, 80 clipped to qy + qh = 60
        (2, 40, 20, 80, 60),          # centre x = 20, exactly on the left edge: kept; x 40 + (0 - 20) 2 = 0 clipped to qx = 40, 80; y 20, 60
        (3, 90, 10, 91, 60),          # 0.5 px wide, 1 px after x2: kept; y 10, 70 clipped to 60.  Row 4 has centre y = 30, on the bottom edge: dropped
        (4, 20, 80, 28, 88),          # tile 2: x 50 * 0.4 = 20, 70 * 0.4 = 28; y 60 + 20, 60 + 28
        (5, 45, 65, 46, 85),          # tile 3: x 40 + 10 / 2, 40 + 12 / 2: 1 px wide, kept; y 60 + 5, 60 + 25
    ], np.float32)
    np.testing.assert_array_equal(got, want)
    # the same tile-3 box one quarter pixel thinner is dropped for extent < 1
    src[3] = np.array([(5, 10, 10, 11.5, 50)], np.float32)
    assert len(D._mosaic_gt(src, m, h, w, 64)[0]) == len(want) - 1
    # the crop's hand-worked cases through tile 0 as a single tile equal the crop's answers
    rows = np.array([r for r, _ in GT_CASES], np.float32)
    single = D.Mosaic([[0, 0, 0, 0]], [[100, 100]], [[WINDOW, (0, 0, 100, 100), (0, 0, 100, 100), (0, 0, 100, 100)]])
    np.testing.assert_array_equal(D._mosaic_gt([rows], single, 100, 100, 64)[0], np.array([wnt for _, wnt in GT_CASES if wnt is not None], np.float32))


def truncating_case():
    """four sources of 20 rows each, all kept by a unit-scale mosaic cut at (50, 50) of a 100 x 100 image, labels 1..80 in visiting
    order -> (gt list, mosaic)"""
    from ssdseglib import datacoder as D
    gts = []
    for k in range(4):
        j = np.arange(20, dtype=np.float32)
        x0, y0 = 2 + 2 * (j % 10), 4 + 20 * (j // 10)
        gts.append(np.stack([20 * k + j + 1, x0, y0, x0 + 3 + 0.25 * k, y0 + 5], axis=1).astype(np.float32))
    m = D.Mosaic([[0, 1, 2, 3]] + [[n] * 4 for n in (1, 2, 3)], [[50, 50]] + [[100, 100]] * 3,
                 [[(0, 0, 50, 50)] * 4] + [[(0, 0, 100, 100)] * 4] * 3)
    return gts, m


def test_mosaic_gt_truncates_in_visiting_order():
    from ssdseglib import datacoder as D
    gts, m = truncating_case()
    rows = D._mosaic_gt(gts, m, 100, 100, 64)[0]
    assert rows.shape == (64, 5) and rows[:, 0].tolist() == list(range(1, 65))
    assert len(D._mosaic_gt(gts, m, 100, 100, 130)[0]) == 80
    np.testing.assert_array_equal(rows[60:64, 1:], gts[3][:4, 1:] + np.array([50, 50, 50, 50], np.float32))


def test_random_mosaic():
    from ssdseglib import datacoder as D
    h, w, n = 96, 128, 2000
    a, b = D.random_mosaic(np.random.default_rng(5), n, h, w), D.random_mosaic(np.random.default_rng(5), n, h, w)
    assert isinstance(a, D.Mosaic) and a.index4.shape == (n, 4) and a.split.shape == (n, 2) and a.windows.shape == (n, 4, 4)
    assert a.index4.dtype == np.int32 and a.split.dtype == np.int32 and a.windows.dtype == np.float32
    assert all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ("index4", "split", "windows"))
    assert a.windows.tobytes() != D.random_mosaic(np.random.default_rng(6), n, h, w).windows.tobytes()
    ident = (a.split == np.array([w, h])).all(axis=1)
    assert abs(ident.mean() - 0.5) < 0.06                                     # 2000 draws at p = 0.5: sigma = 0.011
    own = np.arange(n)
    # identity samples exact
    assert (a.index4[ident] == own[ident, None]).all() and (a.windows[ident] == np.array([0, 0, w, h], np.float32)).all()
    # mosaic samples: tile 0 is the sample itself, partners are positions, quadrants at least 1 px
    mixed = ~ident
    assert (a.index4[mixed, 0] == own[mixed]).all() and a.index4.min() >= 0 and a.index4.max() < n
    assert len(np.unique(a.index4[mixed, 1:])) > n // 2
    px, py = a.split[mixed, 0], a.split[mixed, 1]
    assert px.min() >= 1 and px.max() <= w - 1 and py.min() >= 1 and py.max() <= h - 1
    assert px.min() >= round(0.3 * w) - 1 and px.max() <= round(0.7 * w) + 1 and len(np.unique(px)) > 20
    for mosaic, (hh, ww) in ((a, (h, w)), (D.random_mosaic(np.random.default_rng(7), n, 15, 22, 1.0, (0.0, 1.0), (0.01, 40.0)), (15, 22))):
        mosaic.check(hh, ww)                                                  # the C-ABI's ranges, restated below
        win = mosaic.windows.reshape(-1, 4).astype(np.float64)
        assert np.isfinite(win).all() and (win[:, 2] >= 1).all() and (win[:, 2] <= 16 * ww).all() and (win[:, 3] >= 1).all() and (win[:, 3] <= 16 * hh).all()
        assert (np.abs(win[:, 0]) <= 16 * ww).all() and (np.abs(win[:, 1]) <= 16 * hh).all()
        cut = mosaic.split[(mosaic.split != np.array([ww, hh])).any(axis=1)]   # the mosaic samples: every quadrant at least 1 px
        assert len(cut) > n // 3 and (cut >= 1).all() and (cut[:, 0] <= ww - 1).all() and (cut[:, 1] <= hh - 1).all()
        tol = 4 * 16 * max(hh, ww) * 2.0 ** -23                               # inside / containing, up to float32 rounding (as the crop's sampler)
        for o, e, size in ((win[:, 0], win[:, 2], ww), (win[:, 1], win[:, 3], hh)):
            small = e <= size
            assert (o[small] >= 0).all() and (o[small] + e[small] <= size + tol).all()
            assert (o[~small] <= 0).all() and (o[~small] + e[~small] >= size - tol).all()
    # the window is the quadrant over the zoom: qw / s with s in [0.5, 1]
    qw = np.stack([px, w - px, px, w - px], axis=1)
    ratio = a.windows[mixed][:, :, 2] / qw
    assert ratio.min() >= 1 - 1e-6 and ratio.max() <= 2 + 1e-6 and ratio.max() > 1.8
    # probability 0 and 1
    p0, p1 = D.random_mosaic(np.random.default_rng(5), 50, h, w, probability=0.0), D.random_mosaic(np.random.default_rng(5), 50, h, w, probability=1.0)
    assert (p0.split == np.array([w, h])).all() and (p0.index4 == np.arange(50)[:, None]).all() and (p0.windows == np.array([0, 0, w, h], np.float32)).all()
    assert (p1.split[:, 0] < w).all() and (p1.split[:, 1] < h).all()
    # the number of draws does not depend on their outcomes
    for p in (0.0, 0.5, 1.0):
        r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
        D.random_mosaic(r1, 7, h, w, probability=p); D.random_mosaic(r2, 7, h, w, probability=0.3, center=(0.1, 0.2), scale=(2, 3))
        assert r1.uniform() == r2.uniform()
    for bad in (dict(probability=1.5), dict(scale=(0.0, 1.0)), dict(scale=(1.0, 0.5)), dict(center=(0.5, 1.5)), dict(center=0.5)):
        with pytest.raises(ValueError):
            D.random_mosaic(np.random.default_rng(5), 4, h, w, **bad)
    with pytest.raises(ValueError):
        D.random_mosaic(np.random.default_rng(5), 4, 1, w)


def test_mosaic_holder_is_validated():
    from ssdseglib import datacoder as D
    good = identity_mosaic(2, 6, 8)
    cb = _compact(mosaic=good, mosaic_fill=(1, 2, 3, 1))
    assert cb.mosaic is good and cb.mosaic_fill == (1, 2, 3, 1) and _compact().mosaic is None and _compact().mosaic_fill is None
    ds = _dataset(seed=1)
    rb = ds.batch([3, 0], [1, 0], None, mosaic=good, mosaic_fill=(9, 9, 9, 0))
    assert rb.mosaic is good and rb.mosaic_fill == (9, 9, 9, 0) and ds.batch([3, 0]).mosaic is None
    i4, sp, wn = good.index4, good.split, good.windows
    nan = float("nan")

    def windows(second):
        out = wn.copy()
        out[1, 2] = second
        return out

    for bad in [(i4[:1], sp, wn), (i4[:, :3], sp, wn), (i4, sp[:, :1], wn), (i4, sp, wn[:, :3]), (i4, sp, wn.reshape(2, 16)), ("ab", sp, wn),
                ([[0, 1, 2, 0]] * 2, sp, wn), ([[0, -1, 0, 0]] * 2, sp, wn), ([[0, 0.5, 0, 0]] * 2, sp, wn), (i4, [[-1, 0]] * 2, wn),
                (i4, sp, windows((0, nan, 4, 2))), (i4, sp, windows((0, 0, float("inf"), 2))), (i4, sp, windows((0, 0, 0.5, 2)))]:
        with pytest.raises(ValueError):
            D.Mosaic(*bad)
    # what needs the image size is refused by the batch: splits outside the image, windows outside the C-ABI's range (of an
    # empty quadrant too: tile 2 of the identity is empty), another batch size
    for bad in [D.Mosaic(i4, [[9, 6]] * 2, wn), D.Mosaic(i4, [[8, 7]] * 2, wn), D.Mosaic(i4, sp, windows((0, 0, 8, 16 * 6 + 1))),
                D.Mosaic(i4, sp, windows((17 * 8, 0, 8, 6))), D.Mosaic(i4, sp, windows((0, -17 * 6, 8, 6))), identity_mosaic(3, 6, 8), "mosaic", (i4, sp, wn)]:
        with pytest.raises(ValueError):
            _compact(mosaic=bad)
        with pytest.raises(ValueError):
            ds.batch([3, 0], mosaic=bad)
    for bad in [(0, 0, 0), (0, 0, 0, 256), (0.5, 0, 0, 0), "abcd"]:
        with pytest.raises(ValueError):
            _compact(mosaic=good, mosaic_fill=bad)


def test_mosaic_and_crop_exclude_each_other():
    from ssdseglib import datacoder as D
    good, win = identity_mosaic(2, 6, 8), [(0, 0, 8, 6), (1.5, -2, 4, 3)]
    with pytest.raises(ValueError, match="not both"):
        _compact(mosaic=good, crop_windows=win)
    with pytest.raises(ValueError, match="not both"):
        _dataset(seed=1).batch([3, 0], mosaic=good, crop_windows=win)
    with pytest.raises(ValueError, match="not both"):
        _dataset(seed=1, mosaic=dict(probability=0.5), random_crop=dict(probability=0.5))
    with pytest.raises(ValueError, match="not both"):
        D.augmentation_random_crop(_compact(mosaic=good), None, probability=1.0)
    with pytest.raises(ValueError, match="not both"):
        D.augmentation_mosaic(_compact(crop_windows=win), None)


def test_rng_stream_with_the_option_is_the_epoch_plan():
    """ResidentDataset(mosaic=...): the mosaics are drawn after the epoch's plan, so every batch has the index / flip / colour draws
    of mosaic=None with the same seed; without the option nothing is drawn and nothing is attached"""
    from ssdseglib import datacoder as D
    options = dict(probability=0.7, center=(0.4, 0.6), scale=(0.5, 1.5), fill=(124, 116, 104), fill_class=3)
    plain, mixed = _dataset(seed=21, rgb_augmentation=True, mosaic=None), _dataset(seed=21, rgb_augmentation=True, mosaic=options)
    a, b = list(plain), list(mixed)
    plan = D._epoch_plan(np.random.default_rng(21), N, B, True, True, True, False)
    assert len(a) == len(b) == len(plan) == 3
    for ra, rb, (index, flip, draws) in zip(a, b, plan):
        assert np.array_equal(ra.index, index) and np.array_equal(ra.flip, flip) and ra.rgb_draws == draws
        assert np.array_equal(rb.index, index) and np.array_equal(rb.flip, flip) and rb.rgb_draws == draws
        assert ra.mosaic is None and ra.mosaic_fill is None and rb.crop_windows is None
        assert isinstance(rb.mosaic, D.Mosaic) and len(rb.mosaic) == len(rb) and rb.mosaic_fill == (124, 116, 104, 3)
        assert rb.mosaic.index4.max() < len(rb)                               # positions within the batch, not pool slots
    assert any((rb.mosaic.split[:, 0] < 8).any() for rb in b)
    again = list(_dataset(seed=21, rgb_augmentation=True, mosaic=dict(probability=0.7, center=(0.4, 0.6), scale=(0.5, 1.5))))
    assert all(np.array_equal(x.mosaic.windows, y.mosaic.windows) and np.array_equal(x.mosaic.index4, y.mosaic.index4) for x, y in zip(again, b))
    assert again[0].mosaic_fill == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        _dataset(mosaic=dict(zoom=2))
    with pytest.raises(ValueError):
        _dataset(mosaic=dict(aspect=(1, 2)))
    with pytest.raises(ValueError):
        _dataset(mosaic=dict(fill=(0, 0, 256)))
    with pytest.raises(ValueError):
        _dataset(mosaic=dict(probability=2))


def test_augmentation_mosaic():
    from ssdseglib import datacoder as D
    cb = _compact(b=3, rgb_draws=(0.01, 1.0, 1.0, 0.0))
    targets = object()
    crop_state = D._crop_rng.bit_generator.state
    out, t = D.augmentation_mosaic(cb, targets, probability=1.0, fill=(1, 2, 3), fill_class=2)
    assert D._crop_rng.bit_generator.state == crop_state                       # a stream of its own
    assert t is targets and isinstance(out, D.CompactBatch) and out is not cb and cb.mosaic is None
    assert out.images is cb.images and out.rgb_draws == cb.rgb_draws
    assert len(out.mosaic) == 3 and out.mosaic_fill == (1, 2, 3, 2) and (out.mosaic.split[:, 0] < 8).all()
    state = D._aug_rng.bit_generator.state
    coloured, _ = D.augmentation_rgb_channels(out, None)                       # the colour step on top keeps the mosaic
    D._aug_rng.bit_generator.state = state
    assert coloured.mosaic is out.mosaic and coloured.mosaic_fill == out.mosaic_fill and coloured.rgb_draws != cb.rgb_draws
    assert not np.array_equal(D.augmentation_mosaic(cb, probability=1.0)[0].mosaic.windows, out.mosaic.windows)      # fresh draws
    with pytest.raises(ValueError, match="CompactBatch"):
        D.augmentation_mosaic(np.zeros((2, 6, 8, 3), np.float32), {"output-boxes": np.zeros((2, 4, 4), np.float32)})
    with pytest.raises(ValueError):
        D.augmentation_mosaic(cb, aspect=(1, 2))
