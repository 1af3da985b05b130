"""GPU parity of the mosaic augmentation (csrc/mosaic.hip: ssdseg_mosaic_inputs, ssdseg_mosaic_gt) with its host spec
(datacoder._mosaic_resample / _mosaic_gt, pinned on the CPU in tests/test_cpu_mosaic.py).  The kernels follow the spec operation
for operation in float32, so everything is compared for equality: the assembled bytes, class indices, rows and counts; the engine's
buffers after a ResidentBatch with a mosaic, its compact copy and a plain CompactBatch assembled on the host (which pins mosaic ->
flip -> colour); and `fit` on a ResidentDataset(mosaic=...) against `fit` on the recorded compact copies of its batches."""
import ctypes as C

import numpy as np
import pytest

from tests.test_cpu_mosaic import identity_mosaic, truncating_case
from tests.test_cpu_random_crop import GT_CASES, crop_windows
from tests.test_gpu_full_model import SHAPE, build
from tests.test_gpu_input_pipeline import _compile
from tests.test_gpu_random_crop import _filled, _weights
from tests.test_gpu_resident_dataset import _Replay, _recorded, _resident
from tests.test_gpu_rgb_augmentation import HIGH, _f32
from _guard import BODY_WORD, guards, pattern_bytes  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_POOL = 5
FILL, FILL_CLASS = (124, 116, 104), 3


def _lists(index4, split, windows):
    index4, split = np.ascontiguousarray(index4, np.int32), np.ascontiguousarray(split, np.int32)
    windows = np.ascontiguousarray(windows, np.float32)
    return (index4, split, windows), (index4.ctypes.data, split.ctypes.data, windows.ctypes.data_as(C.POINTER(C.c_float)))


def _mosaic_inputs(ctx, src_img, src_idx, n_src, index4, split, windows, fill, fill_class, d_img, d_idx, b, h, w, flip=None, d_flip=None):
    keep, lists = _lists(index4, split, windows)
    flip = None if flip is None else np.ascontiguousarray(flip, np.uint8)
    ctx.call("ssdseg_mosaic_inputs", src_img, src_idx, n_src, *lists, None if fill is None else (C.c_uint8 * 3)(*fill), fill_class,
             None if flip is None else flip.ctypes.data, d_flip, d_img, d_idx, b, h, w)


def _mosaic_gt(ctx, src_gt, src_cnt, n_src, index4, split, windows, d_gt, d_cnt, b, gmax, h, w):
    keep, lists = _lists(index4, split, windows)
    ctx.call("ssdseg_mosaic_gt", src_gt, src_cnt, n_src, *lists, d_gt, d_cnt, b, gmax, h, w)


def _over_pool(n_pool, index4, split, windows, h, w):
    """the C-ABI names pool slots, the host spec positions within a batch: the spec's batch is the pool repeated up to max(b, n_pool)
    samples (position p holds slot p % n_pool, so a slot is its own position), its Mosaic the b samples asked for followed by
    identities -> (the slot of every position, the Mosaic); the first b outputs are the answer"""
    from ssdseglib import datacoder as D
    b, m = len(index4), max(len(index4), n_pool)
    pad = identity_mosaic(m, h, w)
    i4, sp, wn = pad.index4.copy(), pad.split.copy(), pad.windows.copy()
    i4[:b], sp[:b], wn[:b] = index4, split, windows
    return np.arange(m) % n_pool, D.Mosaic(i4, sp, wn)


def _spec_inputs(img, idx, index4, split, windows, fill, fill_class):
    from ssdseglib import datacoder as D
    h, w = (img if img is not None else idx).shape[1:3]
    slots, mosaic = _over_pool(len(img if img is not None else idx), index4, split, windows, h, w)
    a, c = D._mosaic_resample(None if img is None else img[slots], None if idx is None else idx[slots], mosaic, fill or (0, 0, 0), fill_class)
    return a[:len(index4)], c[:len(index4)]


def _spec_gt(gt, cnt, index4, split, windows, h, w, gmax):
    """-> (rows [b][gmax][5] zero-padded, counts)"""
    from ssdseglib import datacoder as D
    slots, mosaic = _over_pool(len(gt), index4, split, windows, h, w)
    rows = D._mosaic_gt([gt[s, :min(max(cnt[s], 0), gmax)] for s in slots], mosaic, h, w, gmax)[:len(index4)]
    want = np.zeros((len(index4), gmax, 5), np.float32)
    for n, r in enumerate(rows):
        want[n, :len(r)] = r
    return want, [len(r) for r in rows]


def _groups(h, w):
    """nine samples in three batches of 3: splits with px in {0, 1, 5, W - 1, W} and py in {0, 1, H - 1, H}, the crop tests' named
    windows (zoom-in, zoom-out with the fill visible, identity, ...) cycling through the tiles, pool slots that repeat and are out of
    order.  The fifth sample is the identity."""
    named = np.array(list(crop_windows(h, w).values()), np.float32)
    splits = [(0, 0), (1, 1), (5, h - 1), (w - 1, h), (w, h), (w, 0), (0, h), (5, 1), (w - 1, h - 1)]
    windows = np.array([[named[(3 * n + 2 * k) % len(named)] for k in range(4)] for n in range(9)], np.float32)
    windows[4, 0] = (0, 0, w, h)
    slots = np.array([[4, 0, 4, 2], [2, 2, 2, 2], [0, 3, 1, 4], [3, 1, 0, 0], [1, 4, 2, 3], [0, 0, 3, 3], [4, 3, 2, 1], [2, 4, 0, 1], [1, 0, 4, 3]], np.int32)
    return [(slots[i:i + 3], np.array(splits[i:i + 3], np.int32), windows[i:i + 3]) for i in (0, 3, 6)]


@pytest.mark.parametrize("h,w,c,misaligned", [(24, 36, 4, False), (15, 22, 3, False), (24, 36, 4, True)],
                         ids=["24x36-dwords", "15x22-per-pixel", "24x36-misaligned-output"])
def test_mosaic_inputs_equals_the_host_spec(ctx, guards, rng, h, w, c, misaligned):
    b = 3
    img = rng.integers(0, 256, (N_POOL, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, c + 2, (N_POOL, h, w)).astype(np.uint8)
    p_img, p_idx = guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8)
    n_img = b * h * w * 3
    # the misaligned form: the image output starts one byte into a poisoned allocation (no dword stores possible)
    whole = guards.out((n_img + 8,), np.uint8) if misaligned else None
    d_img = whole.view(1, (b, h, w, 3)) if misaligned else guards.out((b, h, w, 3), np.uint8)
    d_idx = guards.out((b, h, w), np.uint8)
    d_flip = guards.out((b,), np.uint8)

    def image_bytes():
        if not misaligned:
            return d_img.download()
        raw = whole.download()
        rest = np.concatenate([raw[:1], raw[1 + n_img:]])
        assert rest.tobytes() == np.concatenate([pattern_bytes(BODY_WORD, n_img + 8)[:1], pattern_bytes(BODY_WORD, n_img + 8)[1 + n_img:]]).tobytes()
        return raw[1:1 + n_img].reshape(b, h, w, 3)

    for (index4, split, win), fill, fill_class in zip(_groups(h, w), ((0, 0, 0), FILL, None), (0, FILL_CLASS, 0)):
        want_img, want_idx = _spec_inputs(img, idx, index4, split, win, fill, fill_class)
        if fill == FILL:
            assert want_img[1].tobytes() == img[index4[1, 0]].tobytes() and want_idx[1].tobytes() == idx[index4[1, 0]].tobytes()      # the identity
            assert (want_idx == FILL_CLASS).any() and (want_img == np.array(FILL, np.uint8)).all(axis=-1).any()                      # fill visible
        # image only, mask only: into the poison
        _mosaic_inputs(ctx, p_img, None, N_POOL, index4, split, win, fill, fill_class, d_img, None, b, h, w)
        np.testing.assert_array_equal(image_bytes(), want_img)
        assert len(guards.unwritten(d_idx)) == d_idx.size
        _mosaic_inputs(ctx, None, p_idx, N_POOL, index4, split, win, fill, fill_class, None, d_idx, b, h, w)
        np.testing.assert_array_equal(d_idx.download(), want_idx)
        guards.check()
        # both, over the complement of the right answer: every output byte has to be written
        d_img.upload(~want_img); d_idx.upload(~want_idx)
        _mosaic_inputs(ctx, p_img, p_idx, N_POOL, index4, split, win, fill, fill_class, d_img, d_idx, b, h, w, flip=[1, 0, 1], d_flip=d_flip)
        np.testing.assert_array_equal(image_bytes(), want_img)
        np.testing.assert_array_equal(d_idx.download(), want_idx)
        assert d_flip.download().tolist() == [1, 0, 1]         # the flags are handed on, not applied
        guards.check()
        guards.repoison(whole if misaligned else d_img); guards.repoison(d_idx); guards.repoison(d_flip)


def test_mosaic_across_argument_blocks(ctx, guards, rng):
    """35 samples of 8x8 from a pool of 9, every one with its own split and windows: the lists cross two 16-sample kernel-argument
    blocks; then the rows of the same samples with gmax = 4, so that the truncation happens there too"""
    from ssdseglib import datacoder as D
    b, h, w, n_pool = 35, 8, 8, 9
    img = rng.integers(0, 256, (n_pool, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, 6, (n_pool, h, w)).astype(np.uint8)
    drawn = D.random_mosaic(rng, b, h, w, probability=1.0, center=(0.0, 1.0), scale=(0.3, 3.0))
    index4 = rng.integers(0, n_pool, (b, 4)).astype(np.int32)
    index4[[0, 15, 16, 31, 32, 34]] = [[8, 0, 8, 3], [0, 8, 1, 7], [7, 7, 7, 7], [8, 8, 0, 0], [3, 2, 1, 0], [5, 8, 0, 8]]
    split, win = drawn.split, drawn.windows
    assert len({tuple(r) for r in win.reshape(b, 16).tolist()}) == b and len({tuple(r) for r in split.tolist()}) > 8
    flip = rng.integers(0, 2, b).astype(np.uint8)
    flip[[15, 16, 31, 32]] = [1, 0, 0, 1]
    want_img, want_idx = _spec_inputs(img, idx, index4, split, win, FILL, FILL_CLASS)
    d_img, d_idx, d_flip = guards.out((b, h, w, 3), np.uint8), guards.out((b, h, w), np.uint8), guards.out((b,), np.uint8)
    d_img.upload(~want_img); d_idx.upload(~want_idx)
    _mosaic_inputs(ctx, guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8), n_pool, index4, split, win, FILL, FILL_CLASS, d_img, d_idx,
                   b, h, w, flip=flip, d_flip=d_flip)
    np.testing.assert_array_equal(d_img.download(), want_img)
    np.testing.assert_array_equal(d_idx.download(), want_idx)
    np.testing.assert_array_equal(d_flip.download(), flip)
    # the rows of the same 35 samples
    gmax = 4
    gt = np.zeros((n_pool, gmax, 5), np.float32)
    cnt = np.array([4, 4, 0, 4, 3, 4, 4, 1, 4], np.int32)                        # mostly full: four tiles of them pass gmax
    for s in range(n_pool):
        x0, y0 = rng.uniform(0, 5, cnt[s]), rng.uniform(0, 5, cnt[s])
        gt[s, :cnt[s]] = np.stack([rng.integers(1, 4, cnt[s]), x0, y0, x0 + rng.uniform(1, 3, cnt[s]), y0 + rng.uniform(1, 3, cnt[s])], axis=1)
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    _mosaic_gt(ctx, guards.inp(gt), guards.inp(cnt, dtype=np.int32), n_pool, index4, split, win, d_gt, d_cnt, b, gmax, h, w)
    want, counts = _spec_gt(gt, cnt, index4, split, win, h, w, gmax)
    uncut, _ = _spec_gt(np.concatenate([gt, np.zeros((n_pool, 12, 5), np.float32)], axis=1), cnt, index4, split, win, h, w, 16)
    assert any((uncut[n, gmax:] != 0).any() for n in range(b)) and 0 in counts and gmax in counts        # some sample keeps more than gmax rows
    np.testing.assert_array_equal(d_cnt.download(), counts)
    np.testing.assert_array_equal(d_gt.download(), want)
    guards.check()


def test_mosaic_gt_equals_the_host_spec(ctx, guards):
    gmax, h, w = 64, 100, 100
    n_pool = 9
    gt = np.full((n_pool, gmax, 5), 7.0, np.float32)           # rows past the count hold something a stale copy would show
    cnt = np.zeros(n_pool, np.int32)

    def put(s, rows):
        rows = np.asarray(rows, np.float32).reshape(-1, 5)
        gt[s, :len(rows)] = rows
        cnt[s] = len(rows)

    # slot 0: all 64 rows, centres alternately in the left and in the right half of the image, each with its own coordinates
    k = np.arange(gmax, dtype=np.float32)
    left = np.stack([1 + k % 3, 25 + k * 0.25, 15 + k * 0.125, 45 + k * 0.25, 35 + k * 0.125], axis=1)
    right = np.stack([1 + k % 3, 62 + k * 0.125, 55 + k * 0.125, 72 + k * 0.125, 85 + k * 0.125], axis=1)
    put(0, np.where((k % 2 == 0)[:, None], left, right))
    put(1, np.zeros((0, 5)))                                                    # count 0
    put(2, [[1, 0, 0, 10, 10], [2, 80, 60, 99, 99], [3, 60, 20, 80, 40]])
    put(3, [[2, -5, -5, 120, 130], [1, 19.75, 20, 20.375, 40]])                 # for the identity: a box that sticks out of the image
    put(4, [r for r, _ in GT_CASES])                                            # the crop's hand-worked edge cases
    sources, truncating = truncating_case()                                     # slots 5..8: 20 rows each, all kept -> 80 -> 64
    for s, rows in enumerate(sources):
        put(5 + s, rows)
    whole, crop = (0, 0, w, h), (20, 10, 50, 40)
    index4 = np.array([[5, 6, 7, 8], [3, 0, 0, 0], [0, 1, 2, 4], [4, 4, 4, 4], [0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 2, 3], [0, 3, 4, 0]], np.int32)
    split = np.array([truncating.split[0], (w, h), (40, 60), (50, 50), (37, 21), (50, 50), (0, 0), (w, 0)], np.int32)
    win = np.array([truncating.windows[0], [whole] * 4, [crop, whole, (0, 0, 120, 80), (19.5, 9.25, 50.5, 41)], [crop] * 4,
                    [(10, 5, 60, 60), (30, 30, 60, 60), whole, (-50, -50, 200, 200)], [whole] * 4, [crop, crop, crop, whole],
                    [crop, (0, 0, 200, 50), crop, crop]], np.float32)
    b = len(index4)
    want, counts = _spec_gt(gt, cnt, index4, split, win, h, w, gmax)
    assert counts[0] == 64 and want[0, :, 0].tolist() == list(range(1, 65))     # 80 kept -> the first 64 in visiting order
    assert counts[1] == 2 and want[1, :2].tobytes() == gt[3, :2].tobytes()      # the verbatim identity, sticking out of the image
    assert counts[5] == 0 and counts[6] == 2 and want[6, 0, 1] == -5            # tile 3 is the whole image (split (0, 0)): verbatim too
    assert 0 < counts[2] < 64 and 0 < counts[3] < 64 and 0 < counts[7] < 64 and counts[4] == 64      # (sample 4 is cut at 64 too)
    p_gt, p_cnt = guards.inp(gt), guards.inp(cnt, dtype=np.int32)
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    _mosaic_gt(ctx, p_gt, p_cnt, n_pool, index4, split, win, d_gt, d_cnt, b, gmax, h, w)
    np.testing.assert_array_equal(d_cnt.download(), counts)                     # counts exact
    np.testing.assert_array_equal(d_gt.download(), want)                        # rows, their order, zeros past the count
    assert len(guards.unwritten(d_gt)) == 0
    guards.check()
    # more rows than one wave: a 130-row source in two of the tiles, so the groups of 64 and the running base are exercised
    big = np.concatenate([gt[0], gt[0, ::-1], gt[0, :2]])[None]
    big = np.concatenate([big, np.zeros_like(big)])
    big[1, :3] = gt[2, :3]
    cnt2 = np.array([130, 3], np.int32)
    i4, sp = np.array([[0, 1, 0, 1]], np.int32), np.array([(45, 52)], np.int32)
    wn = np.array([[(0, 0, 45, 100), whole, (50, 40, 50, 60), whole]], np.float32)
    want, counts = _spec_gt(big, cnt2, i4, sp, wn, h, w, 130)
    assert 64 < counts[0] < 130
    d_gt, d_cnt = guards.out((1, 130, 5)), guards.out((1,), np.int32)
    _mosaic_gt(ctx, guards.inp(big), guards.inp(cnt2, dtype=np.int32), 2, i4, sp, wn, d_gt, d_cnt, 1, 130, h, w)
    assert d_cnt.download().tolist() == counts
    np.testing.assert_array_equal(d_gt.download(), want)
    guards.check()


def test_mosaic_rejects_bad_arguments_before_anything_is_written(ctx, guards):
    from ssdseglib import _hip as H
    b, h, w, gmax = 2, 4, 8, 3
    p_img, p_idx = guards.inp(np.zeros((N_POOL, h, w, 3), np.uint8)), guards.inp(np.zeros((N_POOL, h, w), np.uint8))
    p_gt, p_cnt = guards.inp(np.zeros((N_POOL, gmax, 5), np.float32)), guards.inp(np.ones(N_POOL, np.int32), dtype=np.int32)
    d_img, d_idx, d_flip = guards.out((b, h, w, 3), np.uint8), guards.out((b, h, w), np.uint8), guards.out((b,), np.uint8)
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    whole, small = (0, 0, w, h), (1, 1, 4, 2)
    good_index, good_split, good = [[1, 0, 4, 2], [0, 0, 3, 1]], [(w, h), (3, 2)], [[whole] * 4, [small, whole, small, whole]]
    nan = float("nan")

    def second(window, k=3):
        out = [list(good[0]), list(good[1])]
        out[1][k] = window
        return out

    cases = [   # (index4, split, windows, the argument the error names in both calls)
        ([[1, 0, 4, 2], [0, 0, N_POOL, 1]], good_split, good, 5), ([[1, 0, 4, 2], [0, -1, 3, 1]], good_split, good, 5),
        (good_index, [(w, h), (w + 1, 2)], good, 6), (good_index, [(w, h), (3, h + 1)], good, 6), (good_index, [(w, h), (-1, 2)], good, 6),
        (good_index, [(w, h), (3, -1)], good, 6),
        (good_index, good_split, second((0, nan, 4, 2)), 7), (good_index, good_split, second((0, 0, float("inf"), 2)), 7),
        (good_index, good_split, second((0, 0, 0.5, 2)), 7), (good_index, good_split, second((0, 0, 4, 16 * h + 1)), 7),
        (good_index, good_split, second((17 * w, 0, 4, 2)), 7), (good_index, good_split, second((0, -17 * h, 4, 2)), 7),
        # the window of an EMPTY quadrant (sample 0 has split (W, H): its tile 2 is empty) is checked too
        (good_index, good_split, [[whole, whole, (0, 0, 0.5, 2), whole], good[1]], 7), (good_index, good_split, [[whole, (nan, 0, 4, 2), whole, whole], good[1]], 7),
    ]
    for index4, split, win, arg in cases:
        with pytest.raises(H.SsdsegError, match=f"ssdseg_mosaic_inputs: invalid argument {arg} "):
            _mosaic_inputs(ctx, p_img, p_idx, N_POOL, index4, split, win, FILL, 0, d_img, d_idx, b, h, w, flip=[1, 0], d_flip=d_flip)
        with pytest.raises(H.SsdsegError, match=f"ssdseg_mosaic_gt: invalid argument {arg} "):
            _mosaic_gt(ctx, p_gt, p_cnt, N_POOL, index4, split, win, d_gt, d_cnt, b, gmax, h, w)
    args = (good_index, good_split, good)
    for fill_class in (256, -1):
        with pytest.raises(H.SsdsegError, match="ssdseg_mosaic_inputs: invalid argument 9 "):
            _mosaic_inputs(ctx, p_img, p_idx, N_POOL, *args, FILL, fill_class, d_img, d_idx, b, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 2 "):
        _mosaic_inputs(ctx, None, None, N_POOL, *args, FILL, 0, d_img, d_idx, b, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 11 "):
        _mosaic_inputs(ctx, p_img, p_idx, N_POOL, *args, FILL, 0, d_img, d_idx, b, h, w, flip=[1, 0], d_flip=None)      # flags and nowhere to put them
    with pytest.raises(H.SsdsegError, match="invalid argument 12 "):
        _mosaic_inputs(ctx, p_img, p_idx, N_POOL, *args, FILL, 0, None, d_idx, b, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 12 "):
        _mosaic_inputs(ctx, p_img, p_idx, N_POOL, *args, FILL, 0, p_img, d_idx, b, h, w)           # aliased
    with pytest.raises(H.SsdsegError, match="invalid argument 13 "):
        _mosaic_inputs(ctx, p_img, p_idx, N_POOL, *args, FILL, 0, d_img, None, b, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 13 "):
        _mosaic_inputs(ctx, p_img, p_idx, N_POOL, *args, FILL, 0, d_img, p_idx, b, h, w)
    keep, lists = _lists(*args)
    for hole in range(3):                                                                          # a missing host list
        holed = [None if i == hole else v for i, v in enumerate(lists)]
        with pytest.raises(H.SsdsegError, match=f"ssdseg_mosaic_inputs: invalid argument {5 + hole} "):
            ctx.call("ssdseg_mosaic_inputs", p_img, p_idx, N_POOL, *holed, (C.c_uint8 * 3)(*FILL), 0, None, None, d_img, d_idx, b, h, w)
        with pytest.raises(H.SsdsegError, match=f"ssdseg_mosaic_gt: invalid argument {5 + hole} "):
            ctx.call("ssdseg_mosaic_gt", p_gt, p_cnt, N_POOL, *holed, d_gt, d_cnt, b, gmax, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 8 "):
        _mosaic_gt(ctx, p_gt, p_cnt, N_POOL, *args, None, d_cnt, b, gmax, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 8 "):
        _mosaic_gt(ctx, p_gt, p_cnt, N_POOL, *args, p_gt, d_cnt, b, gmax, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 9 "):
        _mosaic_gt(ctx, p_gt, p_cnt, N_POOL, *args, d_gt, None, b, gmax, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 9 "):
        _mosaic_gt(ctx, p_gt, p_cnt, N_POOL, *args, d_gt, p_cnt, b, gmax, h, w)
    ctx.sync()
    guards.check()
    for buf in (d_img, d_idx, d_flip, d_gt, d_cnt):          # nothing was launched: every output still holds the poison
        assert len(guards.unwritten(buf)) == buf.size, buf.alloc.name


# ---------------------------------------------------------------- the loaders and fit, on the small model
H_, W_ = SHAPE[:2]
PICK = [4, 0, 2]


def _mosaic3():
    """three samples: four tiles around (50, 40) -- zoom-in, zoom-out with the fill visible, partners out of order --, the identity,
    and a two-tile sample (py = H)"""
    from ssdseglib import datacoder as D
    whole = (0, 0, W_, H_)
    return D.Mosaic([[0, 2, 1, 2], [1, 1, 1, 1], [2, 0, 0, 1]], [(50, 40), (W_, H_), (77, H_)],
                    [[(10.25, 5.5, 64, 48), (-32, -12, 1.5 * W_, 1.25 * H_), (0, 0, 50, 56), (20, 30, 100, 60)], [whole] * 4,
                     [(0, 0, 77, H_), (30.5, 0, 51, H_), whole, whole]])


def test_mosaic_batches_fill_the_step_buffers_alike(ctx, guards, rng):
    """a ResidentBatch with a mosaic == its compact copy == a plain CompactBatch assembled on the host by the spec (same flips and
    draws, no mosaic): mosaic, then flip, then colour -- for every combination of flips and colour draws"""
    import ssdseglib
    from ssdseglib import datacoder as D, _engine as E, _loaders as LD
    E.set_default_context(ctx)
    ds, cb = _resident(rng, 5)
    _, _, model = build(seed=5)
    _compile(model)
    eng = E.engine_for(model, 3, True)
    fill, mosaic = FILL + (FILL_CLASS,), _mosaic3()
    for flip, draws in (([1, 0, 1], None), ([0, 1, 1], _f32(HIGH)), (None, _f32(HIGH)), (None, None)):
        rb = ds.batch(PICK, flip, draws, mosaic=mosaic, mosaic_fill=fill)
        compact = ds.to_compact(rb)
        assert compact.mosaic is mosaic and compact.mosaic_fill == fill and compact.rgb_draws == rb.rgb_draws and compact.crop_windows is None
        assert compact.images.tobytes() == cb.images[PICK].tobytes()                        # the copy holds the samples as they are
        img, idx = D._mosaic_resample(cb.images[PICK], cb.mask_index[PICK], mosaic, FILL, FILL_CLASS)
        gts = D._mosaic_gt([cb.ground_truth[s] for s in PICK], mosaic, H_, W_, 64)
        assert img[1].tobytes() == cb.images[PICK[1]].tobytes() and np.array_equal(gts[1], cb.ground_truth[PICK[1]])      # the identity
        assert img[0].tobytes() != cb.images[PICK[0]].tobytes() and (idx[0] == FILL_CLASS).any()
        host = ssdseglib.datacoder.CompactBatch(img, idx, gts, compact.flip, cb.encoder, rgb_draws=draws)
        got = _filled(eng, LD._ResidentLoader, rb)
        same = _filled(eng, LD._CompactLoader, compact)
        want = _filled(eng, LD._CompactLoader, host)
        assert want["__input__"].any()
        for name in want:
            assert got[name].tobytes() == want[name].tobytes(), ("resident", name, flip, draws)
            assert same[name].tobytes() == want[name].tobytes(), ("compact", name, flip, draws)
    # an all-identity mosaic: the bytes of the batch without one
    ident = identity_mosaic(3, H_, W_)
    flip, draws = [0, 1, 1], _f32(HIGH)
    plain = _filled(eng, LD._ResidentLoader, ds.batch(PICK, flip, draws))
    for loader, batch in ((LD._ResidentLoader, ds.batch(PICK, flip, draws, mosaic=ident, mosaic_fill=fill)),
                          (LD._CompactLoader, ds.to_compact(ds.batch(PICK, flip, draws, mosaic=ident)))):
        got = _filled(eng, loader, batch)
        for name in plain:
            assert got[name].tobytes() == plain[name].tobytes(), name
    # and a batch without a mosaic after one with: the loader is back on its old path
    again = _filled(eng, LD._ResidentLoader, ds.batch(PICK, flip, draws))
    assert all(again[name].tobytes() == plain[name].tobytes() for name in plain)
    # train_on_batch takes the same objects
    rb = ds.batch([3, 1, 4], [1, 0, 0], _f32(HIGH), mosaic=mosaic, mosaic_fill=fill)
    logs = model.train_on_batch(rb)
    _, _, model2 = build(seed=5)
    _compile(model2)
    assert logs == model2.train_on_batch(ds.to_compact(rb))


MOSAIC = dict(probability=0.7, center=(0.3, 0.7), scale=(0.5, 1.0), fill=FILL, fill_class=0)


def test_fit_on_a_mosaic_resident_dataset_equals_fit_on_its_compact_batches(ctx, guards):
    """7 samples in batches of 3, 3, 1, flips, colour and the mosaic on, two epochs: the history and the final weights of fit(ds) are
    those of fit over the recorded compact copies (mosaic attached) of the same batches, and not those of the fit without it"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    plans, train = _recorded(1993, 7, seed=11, rgb_augmentation=True, mosaic=MOSAIC)
    assert [[len(rb) for rb in plan] for plan in plans] == [[3, 3, 1], [3, 3, 1]]
    splits = np.concatenate([rb.mosaic.split for plan in plans for rb in plan])
    identity = (splits == np.array([W_, H_])).all(axis=1)
    assert identity.any() and not identity.all() and all(cb.mosaic is not None and cb.mosaic_fill == FILL + (0,) for ep in train for cb in ep)
    _, _, model = build(seed=5)
    _compile(model)
    want = model.fit(_Replay(train), epochs=2, verbose=0).history
    want_weights = _weights(model)
    ds, _ = _resident(np.random.default_rng(1993), 7, seed=11, rgb_augmentation=True, mosaic=MOSAIC)
    _, _, model = build(seed=5)
    _compile(model)
    got = model.fit(ds, epochs=2, verbose=0).history
    assert len(want["loss"]) == 2 and got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    got_weights = _weights(model)
    assert len(got_weights) == len(want_weights) > 100
    for a, b in zip(got_weights, want_weights):
        assert a.tobytes() == b.tobytes()
    # the mosaic matters: the same fit without it gives another history
    plain, _ = _resident(np.random.default_rng(1993), 7, seed=11, rgb_augmentation=True)
    _, _, model = build(seed=5)
    _compile(model)
    assert model.fit(plain, epochs=1, verbose=0).history["loss"][0] != want["loss"][0]


def test_evaluate_on_device_refuses_a_mosaic_batch(ctx, guards, rng):
    import ssdseglib
    from ssdseglib import _engine as E, _fit
    E.set_default_context(ctx)
    ds, _ = _resident(rng, 3, flip=False)
    _, builder, model = build(seed=5)
    inference = builder.get_model_for_inference(model_trained=model, boxes_iou_threshold=0.5, labels_probability_threshold=0.5,
                                                use_segmentation_suppression=False, max_number_of_boxes_per_class=8,
                                                max_number_of_boxes_per_sample=20, suppress_background_boxes=False)
    rb = ds.batch([0, 1, 2], mosaic=_mosaic3())
    for data in ([rb], [ds.to_compact(rb)], iter([rb])):
        with pytest.raises(ValueError, match="mosaic"):
            ssdseglib.evaluators.evaluate_on_device(inference, data, [0, 1, 2, 3], 0, [0.5])
    with pytest.raises(ValueError, match="a mosaic"):
        _fit.run_evaluate(inference, rb, [(0.5, 0.5)])                  # the engine's own door is shut too
