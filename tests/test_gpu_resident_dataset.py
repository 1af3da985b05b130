"""GPU parity of the device-resident training set (datacoder.ResidentDataset; reference NB03#cell8: shuffle, read_and_encode
datacoder.py:302-347, batch, augmentation_rgb_channels :434-466).  ssdseg_gather_inputs / ssdseg_gather_gt (csrc/inputs.hip) build
a batch from pools by sample index; byte / index work, so everything is compared bit for bit: with the oracle's expand_inputs /
flip_gt_boxes on the host-gathered samples, with the merged ssdseg_rgb_augment on the host-stacked pixels (the colour form), with
_CompactLoader on `ds.to_compact(batch)` (the engine's buffers) and with `fit` over those compact batches (the history)."""
import copy
import ctypes as C

import numpy as np
import pytest

from oracle import np_ops as O
from tests.test_gpu_full_model import SHAPE, build
from tests.test_gpu_input_pipeline import B_BLOCKS, BLOCK_SHAPES, ODD_SHAPE, PLACEMENTS, Shifted, _block_flags, _compact_batches, _compile
from tests.test_gpu_rgb_augmentation import CLAMP, HIGH, LOW, _f32, _host as _host_spec, _pixels, _tolerance
from _guard import guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_POOL = 5
ORDER = [4, 0, 4, 2, 0, 3, 1]       # out of order, both ends of the pool, repeats; [:b] for a batch of b
SHAPES = [(3, 7, 13, 4), (7, 9, 16, 3), (1, 5, 5, 8), (4, 48, 64, 4)]       # scalar width; 4-pixel width, b > n_pool; generic c; c == 4


def _host(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _gather_inputs(ctx, pool_img, pool_idx, n_pool, index, flip, draws, means, out_img, out_mask, b, h, w, c):
    index, flip = _host(index, np.int32), _host(flip, np.uint8)
    ctx.call("ssdseg_gather_inputs", pool_img, pool_idx, n_pool, None if index is None else index.ctypes.data,
             None if flip is None else flip.ctypes.data, None if draws is None else (C.c_float * 4)(*draws), means, out_img, out_mask, b, h, w, c)


def _gather_gt(ctx, pool_gt, pool_cnt, n_pool, index, flip, gt, cnt, b, gmax, width):
    index, flip = _host(index, np.int32), _host(flip, np.uint8)
    ctx.call("ssdseg_gather_gt", pool_gt, pool_cnt, n_pool, index.ctypes.data, None if flip is None else flip.ctypes.data, gt, cnt, b, gmax, width)


@pytest.mark.parametrize("b,h,w,c", SHAPES)
def test_gather_inputs_bit_exact(ctx, guards, rng, b, h, w, c):
    img = rng.integers(0, 256, (N_POOL, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, c + 2, (N_POOL, h, w)).astype(np.uint8)       # c, c + 1: out of range -> all-zero one-hot rows
    index = np.array(ORDER[:b], np.int32)
    flip = (np.arange(b) % 2 == 0).astype(np.uint8)
    p_img, p_idx = guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8)
    d_img, d_mask = guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    for f in (flip, None):
        want_img, want_mask = O.expand_inputs(img[index], idx[index], f, c)
        _gather_inputs(ctx, p_img, p_idx, N_POOL, index, f, None, None, d_img, d_mask, b, h, w, c)
        np.testing.assert_array_equal(d_img.download(), want_img)
        np.testing.assert_array_equal(d_mask.download(), want_mask)
        guards.check()
        guards.repoison(d_img); guards.repoison(d_mask)
        # either half alone
        _gather_inputs(ctx, p_img, None, N_POOL, index, f, None, None, d_img, None, b, h, w, c)
        _gather_inputs(ctx, None, p_idx, N_POOL, index, f, None, None, None, d_mask, b, h, w, c)
        np.testing.assert_array_equal(d_img.download(), want_img)
        np.testing.assert_array_equal(d_mask.download(), want_mask)
        guards.check()
        guards.repoison(d_img); guards.repoison(d_mask)


@pytest.mark.parametrize("draws", [LOW, HIGH, CLAMP])
@pytest.mark.parametrize("b,h,w,c", SHAPES)
def test_gather_inputs_colour_form_equals_rgb_augment(ctx, guards, rng, b, h, w, c, draws):
    """the yardstick is the merged entry point on the host-stacked samples: no tolerance, means included"""
    draws = _f32(draws)
    img = _pixels(rng, N_POOL, h, w)
    idx = rng.integers(0, c + 2, (N_POOL, h, w)).astype(np.uint8)
    index = np.array(ORDER[:b], np.int32)
    flip = (np.arange(b) % 2 == 1).astype(np.uint8)
    want_means, want_img = guards.out((b, 3)), guards.out((b, h, w, 3))
    ctx.call("ssdseg_rgb_augment", guards.inp(img[index], dtype=np.uint8), guards.inp(flip, dtype=np.uint8), (C.c_float * 4)(*draws), want_means,
             want_img, b, h, w)
    _, want_mask = O.expand_inputs(img[index], idx[index], flip, c)
    p_img, p_idx = guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8)
    means, d_img, d_mask = guards.out((b, 3)), guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    _gather_inputs(ctx, p_img, p_idx, N_POOL, index, flip, draws, means, d_img, d_mask, b, h, w, c)
    assert means.download().tobytes() == want_means.download().tobytes()
    assert d_img.download().tobytes() == want_img.download().tobytes()
    np.testing.assert_array_equal(d_mask.download(), want_mask)
    guards.check()
    guards.repoison(means); guards.repoison(d_img)
    _gather_inputs(ctx, p_img, None, N_POOL, index, flip, draws, means, d_img, None, b, h, w, c)       # the image half alone
    assert means.download().tobytes() == want_means.download().tobytes()
    assert d_img.download().tobytes() == want_img.download().tobytes()


def test_gather_gt_bit_exact(ctx, guards, rng):
    gmax, width, b = 6, 640.0, 7
    cnt = np.array([0, gmax, 3, 2, 5], np.int32)
    gt = np.full((N_POOL, gmax, 5), 7.0, np.float32)            # rows past the count hold something a stale copy would show
    for s in range(N_POOL):
        x0 = rng.uniform(0, 500, cnt[s]); x1 = x0 + rng.uniform(1, 139, cnt[s])
        gt[s, :cnt[s]] = np.stack([rng.integers(1, 4, cnt[s]), x0, rng.uniform(0, 400, cnt[s]), x1, rng.uniform(400, 479, cnt[s])], axis=1)
    index = np.array(ORDER[:b], np.int32)
    flip = np.array([1, 1, 0, 1, 0, 1, 0], np.uint8)
    p_gt, p_cnt = guards.inp(gt), guards.inp(cnt, dtype=np.int32)
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    for f in (flip, None):
        want = np.zeros((b, gmax, 5), np.float32)
        for n, s in enumerate(index):
            rows = gt[s, :cnt[s]]
            want[n, :cnt[s]] = O.flip_gt_boxes(rows, width) if f is not None and f[n] else rows
        _gather_gt(ctx, p_gt, p_cnt, N_POOL, index, f, d_gt, d_cnt, b, gmax, width)
        np.testing.assert_array_equal(d_cnt.download(), cnt[index])
        got = d_gt.download()
        np.testing.assert_array_equal(got, want)
        assert all(not got[n, cnt[s]:].any() for n, s in enumerate(index))      # rows past the count are zeros
        guards.check()
        guards.repoison(d_gt); guards.repoison(d_cnt)


POOL_BLOCKS = 9


def _block_lists(rng):
    """index list and flags of B_BLOCKS samples: both ends of the pool on either side of both 64-sample block edges and at the
    end of the list, flags that differ across the edges"""
    index = rng.integers(0, POOL_BLOCKS, B_BLOCKS).astype(np.int32)
    index[[0, 63, 64, 127, 128, 129]] = [8, 0, 8, 0, 8, 0]
    return index, _block_flags(rng)


@pytest.mark.parametrize("h,w,c", BLOCK_SHAPES)
def test_gather_inputs_across_argument_blocks(ctx, guards, rng, h, w, c):
    b = B_BLOCKS
    img = _pixels(rng, POOL_BLOCKS, h, w)
    idx = rng.integers(0, c + 2, (POOL_BLOCKS, h, w)).astype(np.uint8)
    index, flip = _block_lists(rng)
    p_img, p_idx = guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8)
    d_img, d_mask = guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    want_img, want_mask = O.expand_inputs(img[index], idx[index], flip, c)
    _gather_inputs(ctx, p_img, p_idx, POOL_BLOCKS, index, flip, None, None, d_img, d_mask, b, h, w, c)
    np.testing.assert_array_equal(d_img.download(), want_img)
    np.testing.assert_array_equal(d_mask.download(), want_mask)
    guards.check()
    guards.repoison(d_img); guards.repoison(d_mask)
    # the colour form: the merged entry point on the host-stacked samples byte for byte, and the host spec within its bound
    draws = _f32(HIGH)
    want_means, want_aug = guards.out((b, 3)), guards.out((b, h, w, 3))
    ctx.call("ssdseg_rgb_augment", guards.inp(img[index], dtype=np.uint8), guards.inp(flip, dtype=np.uint8), (C.c_float * 4)(*draws), want_means,
             want_aug, b, h, w)
    means = guards.out((b, 3))
    _gather_inputs(ctx, p_img, p_idx, POOL_BLOCKS, index, flip, draws, means, d_img, d_mask, b, h, w, c)
    assert means.download().tobytes() == want_means.download().tobytes()
    assert d_img.download().tobytes() == want_aug.download().tobytes()
    np.testing.assert_array_equal(d_mask.download(), want_mask)
    guards.check()
    spec, m64, m32 = _host_spec(img[index], flip, draws)
    np.testing.assert_allclose(means.download(), m64, rtol=1e-5)
    err = float(np.abs(d_img.download() - spec).max())
    assert err <= _tolerance(draws, m64, m32), (err, _tolerance(draws, m64, m32))


def test_gather_gt_across_argument_blocks(ctx, guards, rng):
    gmax, width, b = 4, 640.0, B_BLOCKS
    cnt = np.array([gmax, 0, 3, 2, 1, gmax, 0, 2, 3], np.int32)
    gt = np.full((POOL_BLOCKS, gmax, 5), 7.0, np.float32)       # rows past the count hold something a stale copy would show
    for s in range(POOL_BLOCKS):
        x0 = rng.uniform(0, 500, cnt[s]); x1 = x0 + rng.uniform(1, 139, cnt[s])
        gt[s, :cnt[s]] = np.stack([rng.integers(1, 4, cnt[s]), x0, rng.uniform(0, 400, cnt[s]), x1, rng.uniform(400, 479, cnt[s])], axis=1)
    index, flip = _block_lists(rng)
    want = np.zeros((b, gmax, 5), np.float32)
    for n, s in enumerate(index):
        rows = gt[s, :cnt[s]]
        want[n, :cnt[s]] = O.flip_gt_boxes(rows, width) if flip[n] else rows
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    _gather_gt(ctx, guards.inp(gt), guards.inp(cnt, dtype=np.int32), POOL_BLOCKS, index, flip, d_gt, d_cnt, b, gmax, width)
    np.testing.assert_array_equal(d_cnt.download(), cnt[index])
    got = d_gt.download()
    np.testing.assert_array_equal(got, want)
    assert all(not got[n, cnt[s]:].any() for n, s in enumerate(index))      # rows past the count are zeros
    guards.check()


@pytest.mark.parametrize("which", PLACEMENTS)
def test_gather_inputs_falls_back_on_a_misaligned_buffer(ctx, guards, rng, which):
    """both forms; the pools are the shifted sources"""
    b, h, w, c = ODD_SHAPE
    img = _pixels(rng, N_POOL, h, w)
    idx = rng.integers(0, c + 2, (N_POOL, h, w)).astype(np.uint8)
    index, flip = np.array([4, 0], np.int32), np.array([1, 0], np.uint8)
    want_img, want_mask = O.expand_inputs(img[index], idx[index], flip, c)
    p_img, p_idx = guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8)
    a_means, a_img, a_mask = guards.out((b, 3)), guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    s, means = Shifted(guards, img, idx, which, b, c), guards.out((b, 3))
    _gather_inputs(ctx, p_img, p_idx, N_POOL, index, flip, None, None, a_img, a_mask, b, h, w, c)
    _gather_inputs(ctx, s.img, s.idx, N_POOL, index, flip, None, None, s.out, s.mask_out, b, h, w, c)
    assert s.image().tobytes() == a_img.download().tobytes() == want_img.tobytes()
    assert s.mask().tobytes() == a_mask.download().tobytes() == want_mask.tobytes()
    guards.check()
    s.repoison(guards); guards.repoison(a_img); guards.repoison(a_mask)
    draws = _f32(HIGH)
    _gather_inputs(ctx, p_img, p_idx, N_POOL, index, flip, draws, a_means, a_img, a_mask, b, h, w, c)
    _gather_inputs(ctx, s.img, s.idx, N_POOL, index, flip, draws, means, s.out, s.mask_out, b, h, w, c)
    assert s.image().tobytes() == a_img.download().tobytes() and means.download().tobytes() == a_means.download().tobytes()
    assert s.mask().tobytes() == a_mask.download().tobytes() == want_mask.tobytes()
    guards.check()
    spec, m64, m32 = _host_spec(img[index], flip, draws)
    np.testing.assert_allclose(a_means.download(), m64, rtol=1e-5)
    assert float(np.abs(a_img.download() - spec).max()) <= _tolerance(draws, m64, m32)


def test_gather_rejects_bad_arguments_before_anything_is_written(ctx, guards):
    from ssdseglib import _hip as H
    b, h, w, c = 2, 2, 4, 4
    p_img = guards.inp(np.zeros((N_POOL, h, w, 3), np.uint8))
    p_idx = guards.inp(np.zeros((N_POOL, h, w), np.uint8))
    means, d_img, d_mask = guards.out((b, 3)), guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    good, ident, nan = [1, 0], (0.0, 1.0, 1.0, 0.0), (0.0, float("nan"), 1.0, 0.0)
    bad_calls = [
        dict(index=[0, -1]), dict(index=[N_POOL, 0]), dict(b=0), dict(c=9),
        dict(draws=ident, means=None),                       # draws without means
        dict(draws=nan),
        dict(pool_img=None, pool_idx=None),                  # nothing to gather
        dict(d_img=None), dict(d_mask=None),                 # a pool without its destination
        dict(pool_img=None, d_img=None, draws=ident),        # draws without the image pair
    ]
    for kw in bad_calls:
        a = dict(pool_img=p_img, pool_idx=p_idx, index=good, draws=None, means=means, d_img=d_img, d_mask=d_mask, b=b, c=c)
        a.update(kw)
        with pytest.raises(H.SsdsegError):
            _gather_inputs(ctx, a["pool_img"], a["pool_idx"], N_POOL, a["index"], [1, 0], a["draws"], a["means"], a["d_img"], a["d_mask"],
                           a["b"], h, w, a["c"])
    p_gt, p_cnt = guards.inp(np.zeros((N_POOL, 3, 5), np.float32)), guards.inp(np.ones(N_POOL, np.int32), dtype=np.int32)
    d_gt, d_cnt = guards.out((b, 3, 5)), guards.out((b,), np.int32)
    for index, bb in (([0, -1], b), ([N_POOL, 0], b), (good, 0)):
        with pytest.raises(H.SsdsegError):
            _gather_gt(ctx, p_gt, p_cnt, N_POOL, index, [1, 0], d_gt, d_cnt, bb, 3, 640.0)
    ctx.sync()
    guards.check()
    for buf in (means, d_img, d_mask, d_gt, d_cnt):          # nothing was launched: every output still holds the poison
        assert len(guards.unwritten(buf)) == buf.size, buf.alloc.name


def _encoder(shape, flip=False):
    import ssdseglib
    z = np.zeros(4, np.float32)
    return ssdseglib.datacoder.DataEncoderDecoder(4, shape, xmin_boxes_default=z, ymin_boxes_default=z, xmax_boxes_default=z + 9,
                                                  ymax_boxes_default=z + 9, augmentation_horizontal_flip=flip)


def test_pool_offsets_past_4_gib(ctx, guards, rng):
    """4,661 samples of 480x640: the image pool is 4,295,577,600 bytes, so the last sample starts past 2^31 and runs across 2^32
    (its byte 311,296 is pool byte 2^32).  Two slots are written."""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    h, w, c, cap = 480, 640, 4, 4661
    ds = ssdseglib.datacoder.ResidentDataset(_encoder((h, w)), capacity=cap)
    img = _pixels(rng, 2, h, w)
    idx = rng.integers(0, c + 2, (2, h, w)).astype(np.uint8)
    gts = [np.array([[1, 10, 20, 110, 220]], np.float32), np.array([[2, 5, 6, 70, 80], [3, 300, 200, 639, 479]], np.float32)]
    ds.write(0, img[0], idx[0], gts[0])
    ds.write(cap - 1, img[1], idx[1], gts[1])
    assert ds.num_samples == cap and ds.images.nbytes == 4295577600
    assert 1 << 31 < (cap - 1) * h * w * 3 < 1 << 32 < cap * h * w * 3
    index, flip, pick = np.array([cap - 1, 0], np.int32), np.array([1, 0], np.uint8), [1, 0]
    want_img, want_mask = O.expand_inputs(img[pick], idx[pick], flip, c)
    d_img, d_mask = guards.out((2, h, w, 3)), guards.out((2, h, w, c))
    _gather_inputs(ctx, ds.images, ds.masks, cap, index, flip, None, None, d_img, d_mask, 2, h, w, c)
    np.testing.assert_array_equal(d_img.download(), want_img)
    np.testing.assert_array_equal(d_mask.download(), want_mask)
    # the colour form reads the pool through the same offsets
    draws = _f32(HIGH)
    want_means, want_aug = guards.out((2, 3)), guards.out((2, h, w, 3))
    ctx.call("ssdseg_rgb_augment", guards.inp(img[pick], dtype=np.uint8), guards.inp(flip, dtype=np.uint8), (C.c_float * 4)(*draws), want_means,
             want_aug, 2, h, w)
    means = guards.out((2, 3))
    guards.repoison(d_img)
    _gather_inputs(ctx, ds.images, None, cap, index, flip, draws, means, d_img, None, 2, h, w, c)
    assert means.download().tobytes() == want_means.download().tobytes()
    assert d_img.download().tobytes() == want_aug.download().tobytes()
    d_gt, d_cnt = guards.out((2, ds.GMAX, 5)), guards.out((2,), np.int32)
    _gather_gt(ctx, ds.gt, ds.cnt, cap, index, flip, d_gt, d_cnt, 2, ds.GMAX, float(w))
    assert d_cnt.download().tolist() == [2, 1]
    np.testing.assert_array_equal(d_gt.download()[0, :2], O.flip_gt_boxes(gts[1], w))
    np.testing.assert_array_equal(d_gt.download()[1, :1], gts[0])
    cb = ds.to_compact(ds.batch(index, flip))
    assert cb.images.tobytes() == img[pick].tobytes() and cb.mask_index.tobytes() == idx[pick].tobytes()


def _resident(rng, n, flip=True, **kw):
    """n samples of the small model's shape in a ResidentDataset (and the encoder's compact batch they came from)"""
    import ssdseglib
    (cb, _, _), = _compact_batches(rng, (n,))
    enc = copy.copy(cb.encoder)
    enc.augmentation_horizontal_flip = flip
    samples = list(zip(cb.images, cb.mask_index, cb.ground_truth, cb.flip))
    return ssdseglib.datacoder.ResidentDataset(enc, samples, batch_size=3, **kw), cb


def _buffers(eng):
    out = {"__input__": eng.input_store.buf.download()}
    for name, op, kind in eng._loss_names:
        buf = op.y_true if kind == "mask" else (op.y_labels if kind == "conf" else op.y_boxes)
        out[name] = buf.download()
        buf.zero_()
    eng.input_store.buf.zero_()
    return out


def test_resident_batch_fills_the_step_buffers_like_its_compact_copy(ctx, guards, rng):
    from ssdseglib import _engine as E, _loaders as LD
    E.set_default_context(ctx)
    ds, cb = _resident(rng, 5)
    assert ds.num_samples == 5 and len(ds) == 2
    _, _, model = build(seed=5)
    _compile(model)
    eng = E.engine_for(model, 3, True)
    for flip, draws in (([1, 0, 1], None), ([0, 1, 1], _f32(HIGH)), (None, _f32(CLAMP)), ([0, 0, 0], None)):
        rb = ds.batch(ORDER[:3], flip, draws)
        compact = ds.to_compact(rb)
        assert compact.images.tobytes() == cb.images[ORDER[:3]].tobytes() and compact.mask_index.tobytes() == cb.mask_index[ORDER[:3]].tobytes()
        assert all(np.array_equal(g, cb.ground_truth[s]) for g, s in zip(compact.ground_truth, ORDER[:3]))
        assert compact.rgb_draws == rb.rgb_draws and compact.flip.tolist() == (flip or [0, 0, 0])
        ld = LD.loader_for(eng, rb)
        assert type(ld) is LD._ResidentLoader
        ld.stage(rb)
        ld.consume()
        got = _buffers(eng)
        ld = LD.loader_for(eng, compact)
        assert type(ld) is LD._CompactLoader
        ld.stage(compact)
        ld.consume()
        want = _buffers(eng)
        assert want["__input__"].any()
        for name in want:
            assert got[name].tobytes() == want[name].tobytes(), (name, flip, draws)
    # train_on_batch takes the same object
    rb = ds.batch([3, 1, 4], [1, 0, 0], _f32(LOW))
    logs = model.train_on_batch(rb)
    _, _, model2 = build(seed=5)
    _compile(model2)
    assert logs == model2.train_on_batch(ds.to_compact(rb))


def test_resident_loader_checks_the_encoder_like_the_compact_loader(ctx, guards, rng):
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    ds, cb = _resident(rng, 2)
    enc5 = copy.copy(ds.encoder)
    enc5.num_classes = 5
    wrong = ssdseglib.datacoder.ResidentDataset(enc5, zip(cb.images, cb.mask_index, cb.ground_truth))
    _, _, model = build(seed=5)
    _compile(model)
    with pytest.raises(ValueError, match="num_classes"):
        model.train_on_batch(wrong.batch([0, 1]))
    with pytest.raises(ValueError, match="64"):
        ds.write(0, cb.images[0], cb.mask_index[0], np.tile(cb.ground_truth[0][:1], (65, 1)))
    with pytest.raises(ValueError):
        ds.write(0, cb.images[0][:-1], cb.mask_index[0], cb.ground_truth[0])
    with pytest.raises(IndexError):
        ds.write(2, cb.images[0], cb.mask_index[0], cb.ground_truth[0])


class _Replay:
    """an iterable whose k-th iteration yields the k-th recorded epoch"""

    def __init__(self, epochs):
        self.epochs = iter(epochs)

    def __iter__(self):
        return iter(next(self.epochs))


def _recorded(rng_seed, n, seed, epochs=2, **kw):
    """the epochs a dataset with this seed will produce, as lists of compact batches (from a twin built from the same samples)"""
    twin, _ = _resident(np.random.default_rng(rng_seed), n, seed=seed, **kw)
    plans = [list(twin) for _ in range(epochs)]
    return plans, [[twin.to_compact(rb) for rb in plan] for plan in plans]


def test_fit_on_a_resident_dataset_equals_fit_on_its_compact_batches(ctx, guards, monkeypatch):
    """7 samples in batches of 3, 3, 1 (the last through an engine of its own), flips and colour on, two epochs with different
    orders: the history of fit(ds) -- overlapped and synchronous -- is the history of fit over the same batches downloaded as
    CompactBatch objects, bit for bit"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    plans, lists = _recorded(1993, 7, seed=11, rgb_augmentation=True)
    assert [[len(rb) for rb in plan] for plan in plans] == [[3, 3, 1], [3, 3, 1]]
    order = [np.concatenate([rb.index for rb in plan]) for plan in plans]
    assert sorted(order[0].tolist()) == sorted(order[1].tolist()) == list(range(7)) and not np.array_equal(order[0], order[1])
    assert any(rb.flip.any() for plan in plans for rb in plan) and all(rb.rgb_draws is not None for plan in plans for rb in plan)
    _, _, model = build(seed=5)
    _compile(model)
    want = model.fit(_Replay(lists), epochs=2, verbose=0).history
    assert len(want["loss"]) == 2
    for overlap in ("1", "0"):
        monkeypatch.setenv("SSDSEG_FIT_OVERLAP", overlap)
        ds, _ = _resident(np.random.default_rng(1993), 7, seed=11, rgb_augmentation=True)
        _, _, model = build(seed=5)
        _compile(model)
        got = model.fit(ds, epochs=2, verbose=0).history
        assert got.keys() == want.keys()
        for k in want:
            assert got[k] == want[k], (overlap, k, got[k], want[k])


def test_fit_validates_on_a_resident_dataset(ctx, guards):
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    _, train = _recorded(1993, 6, seed=11, rgb_augmentation=True)
    _, val = _recorded(7, 4, seed=3, rgb_augmentation=True)
    _, _, model = build(seed=5)
    _compile(model)
    want = model.fit(_Replay(train), epochs=2, validation_data=_Replay(val), verbose=0).history
    ds, _ = _resident(np.random.default_rng(1993), 6, seed=11, rgb_augmentation=True)
    vds, _ = _resident(np.random.default_rng(7), 4, seed=3, rgb_augmentation=True)
    _, _, model = build(seed=5)
    _compile(model)
    got = model.fit(ds, epochs=2, validation_data=vds, verbose=0).history
    assert "val_loss" in want and got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
