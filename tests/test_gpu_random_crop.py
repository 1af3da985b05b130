"""GPU parity of the random crop / zoom-out augmentation (csrc/crop.hip: ssdseg_crop_inputs, ssdseg_crop_gt) with its host spec
(datacoder._crop_resample / _crop_gt, checked on the CPU in tests/test_cpu_random_crop.py).  The kernels follow the spec operation
for operation in float32, so everything is compared for equality: the cropped bytes, class indices, rows and counts; the engine's
buffers after a cropped ResidentBatch, its compact copy and a host-cropped plain CompactBatch (which pins crop -> flip -> colour);
and `fit` on a ResidentDataset(random_crop=...) against `fit` on the recorded compact copies of its batches."""
import ctypes as C

import numpy as np
import pytest

from tests.test_cpu_random_crop import GT_CASES, WINDOW, crop_windows
from tests.test_gpu_full_model import SHAPE, build
from tests.test_gpu_input_pipeline import _compile
from tests.test_gpu_resident_dataset import _Replay, _buffers, _recorded, _resident
from tests.test_gpu_rgb_augmentation import HIGH, _f32
from _guard import BODY_WORD, guards, pattern_bytes  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_POOL = 5
FILL, FILL_CLASS = (124, 116, 104), 3


def _crop_inputs(ctx, src_img, src_idx, n_src, index, windows, fill, fill_class, d_img, d_idx, b, h, w, flip=None, d_flip=None):
    index = None if index is None else np.ascontiguousarray(index, np.int32)
    windows = np.ascontiguousarray(windows, np.float32)
    flip = None if flip is None else np.ascontiguousarray(flip, np.uint8)
    ctx.call("ssdseg_crop_inputs", src_img, src_idx, n_src, None if index is None else index.ctypes.data,
             windows.ctypes.data_as(C.POINTER(C.c_float)), None if fill is None else (C.c_uint8 * 3)(*fill), fill_class,
             None if flip is None else flip.ctypes.data, d_flip, d_img, d_idx, b, h, w)


def _crop_gt(ctx, src_gt, src_cnt, n_src, index, windows, d_gt, d_cnt, b, gmax, h, w):
    index = None if index is None else np.ascontiguousarray(index, np.int32)
    windows = np.ascontiguousarray(windows, np.float32)
    ctx.call("ssdseg_crop_gt", src_gt, src_cnt, n_src, None if index is None else index.ctypes.data,
             windows.ctypes.data_as(C.POINTER(C.c_float)), d_gt, d_cnt, b, gmax, h, w)


def _groups(h, w):
    """the seven named windows in three batches of 3, with pool indices that repeat and are out of order"""
    win = np.array(list(crop_windows(h, w).values()), np.float32)
    return [([4, 0, 4], win[[0, 1, 2]]), ([2, 0, 3], win[[3, 4, 5]]), ([1, 1, 2], win[[6, 0, 3]])]


@pytest.mark.parametrize("h,w,c,misaligned", [(24, 36, 4, False), (15, 22, 3, False), (24, 36, 4, True)],
                         ids=["24x36-dwords", "15x22-per-pixel", "24x36-misaligned-output"])
def test_crop_inputs_equals_the_host_spec(ctx, guards, rng, h, w, c, misaligned):
    from ssdseglib import datacoder as D
    b = 3
    img = rng.integers(0, 256, (N_POOL, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, c + 2, (N_POOL, h, w)).astype(np.uint8)
    p_img, p_idx = guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8)
    n_img, n_idx = b * h * w * 3, b * h * w
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

    for (index, win), fill, fill_class in zip(_groups(h, w), ((0, 0, 0), FILL, None), (0, FILL_CLASS, 0)):
        want_img, want_idx = D._crop_resample(img[index], idx[index], win, fill or (0, 0, 0), fill_class)
        # image only, mask only: into the poison
        _crop_inputs(ctx, p_img, None, N_POOL, index, win, fill, fill_class, d_img, None, b, h, w)
        np.testing.assert_array_equal(image_bytes(), want_img)
        assert len(guards.unwritten(d_idx)) == d_idx.size
        _crop_inputs(ctx, None, p_idx, N_POOL, index, win, fill, fill_class, None, d_idx, b, h, w)
        np.testing.assert_array_equal(d_idx.download(), want_idx)
        guards.check()
        # both, over the complement of the right answer: every output byte has to be written
        d_img.upload(~want_img); d_idx.upload(~want_idx)
        _crop_inputs(ctx, p_img, p_idx, N_POOL, index, win, fill, fill_class, d_img, d_idx, b, h, w, flip=[1, 0, 1], d_flip=d_flip)
        np.testing.assert_array_equal(image_bytes(), want_img)
        np.testing.assert_array_equal(d_idx.download(), want_idx)
        assert d_flip.download().tolist() == [1, 0, 1]         # the flags are handed on, not applied
        guards.check()
        guards.repoison(whole if misaligned else d_img); guards.repoison(d_idx); guards.repoison(d_flip)
    # the compact form (no index list: n -> n) and the identity: the source bytes
    ident = np.tile(np.array([0, 0, w, h], np.float32), (b, 1))
    _crop_inputs(ctx, p_img, p_idx, N_POOL, None, ident, FILL, FILL_CLASS, d_img, d_idx, b, h, w)
    assert image_bytes().tobytes() == img[:b].tobytes() and d_idx.download().tobytes() == idx[:b].tobytes()


def test_crop_inputs_across_argument_blocks(ctx, guards, rng):
    """70 samples of 8x8 from a pool of 9, every one through another window: the lists cross the 64-sample kernel-argument block"""
    from ssdseglib import datacoder as D
    b, h, w, n_pool = 70, 8, 8, 9
    img = rng.integers(0, 256, (n_pool, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, 6, (n_pool, h, w)).astype(np.uint8)
    index = rng.integers(0, n_pool, b).astype(np.int32)
    index[[0, 63, 64, 69]] = [8, 0, 8, 3]
    win = D.random_crop_windows(rng, b, h, w, probability=1.0, scale=(0.3, 3.0))
    assert len({tuple(r) for r in win.tolist()}) == b
    flip = rng.integers(0, 2, b).astype(np.uint8)
    flip[[63, 64]] = [1, 0]
    want_img, want_idx = D._crop_resample(img[index], idx[index], win, FILL, FILL_CLASS)
    d_img, d_idx, d_flip = guards.out((b, h, w, 3), np.uint8), guards.out((b, h, w), np.uint8), guards.out((b,), np.uint8)
    d_img.upload(~want_img); d_idx.upload(~want_idx)
    _crop_inputs(ctx, guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8), n_pool, index, win, FILL, FILL_CLASS, d_img, d_idx, b, h, w,
                 flip=flip, d_flip=d_flip)
    np.testing.assert_array_equal(d_img.download(), want_img)
    np.testing.assert_array_equal(d_idx.download(), want_idx)
    np.testing.assert_array_equal(d_flip.download(), flip)
    # the rows of the same 70 samples
    gmax = 4
    gt = np.zeros((n_pool, gmax, 5), np.float32)
    cnt = rng.integers(0, gmax + 1, n_pool).astype(np.int32)
    for s in range(n_pool):
        x0, y0 = rng.uniform(0, 5, cnt[s]), rng.uniform(0, 5, cnt[s])
        gt[s, :cnt[s]] = np.stack([rng.integers(1, 4, cnt[s]), x0, y0, x0 + rng.uniform(1, 3, cnt[s]), y0 + rng.uniform(1, 3, cnt[s])], axis=1)
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    _crop_gt(ctx, guards.inp(gt), guards.inp(cnt, dtype=np.int32), n_pool, index, win, d_gt, d_cnt, b, gmax, h, w)
    rows = D._crop_gt([gt[s, :cnt[s]] for s in index], win, h, w)
    want = np.zeros((b, gmax, 5), np.float32)
    for n, r in enumerate(rows):
        want[n, :len(r)] = r
    np.testing.assert_array_equal(d_cnt.download(), [len(r) for r in rows])
    np.testing.assert_array_equal(d_gt.download(), want)
    assert 0 < sum(len(r) for r in rows) < int(cnt[index].sum())


def test_crop_gt_equals_the_host_spec(ctx, guards, rng):
    from ssdseglib import datacoder as D
    gmax, h, w = 64, 100, 100
    gt = np.full((N_POOL, gmax, 5), 7.0, np.float32)           # rows past the count hold something a stale copy would show
    cnt = np.zeros(N_POOL, np.int32)

    def put(s, rows):
        rows = np.asarray(rows, np.float32).reshape(-1, 5)
        gt[s, :len(rows)] = rows
        cnt[s] = len(rows)

    # sample 0: all 64 rows, kept and dropped in turn (centre inside WINDOW / left of it), each with its own coordinates
    k = np.arange(gmax, dtype=np.float32)
    inside = np.stack([1 + k % 3, 25 + k * 0.25, 15 + k * 0.125, 45 + k * 0.25, 35 + k * 0.125], axis=1)
    outside = np.stack([1 + k % 3, 2 + k * 0.125, 15 + k * 0.125, 12 + k * 0.125, 35 + k * 0.125], axis=1)
    put(0, np.where((k % 2 == 0)[:, None], inside, outside))
    put(1, np.zeros((0, 5)))                                                    # count 0
    put(2, [[1, 0, 0, 10, 10], [2, 80, 60, 99, 99], [3, 60, 20, 80, 40]])       # loses every row
    put(3, [[2, -5, -5, 120, 130], [1, 19.75, 20, 20.375, 40]])                 # for the identity: a box that sticks out of the image
    put(4, [r for r, _ in GT_CASES])                                            # the hand-worked edge cases
    index = np.array([0, 1, 2, 3, 4, 0, 4], np.int32)
    win = np.array([WINDOW, WINDOW, WINDOW, (0, 0, w, h), WINDOW, (0, 0, w, h), (19.5, 9.25, 50.5, 41)], np.float32)
    b = len(index)
    rows = D._crop_gt([gt[s, :cnt[s]] for s in index], win, h, w)
    assert [len(r) for r in rows][:6] == [32, 0, 0, 2, sum(wnt is not None for _, wnt in GT_CASES), 64]
    want = np.zeros((b, gmax, 5), np.float32)
    for n, r in enumerate(rows):
        want[n, :len(r)] = r
    p_gt, p_cnt = guards.inp(gt), guards.inp(cnt, dtype=np.int32)
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    _crop_gt(ctx, p_gt, p_cnt, N_POOL, index, win, d_gt, d_cnt, b, gmax, h, w)
    np.testing.assert_array_equal(d_cnt.download(), [len(r) for r in rows])     # counts exact
    got = d_gt.download()
    np.testing.assert_array_equal(got, want)                                    # rows, their order, zeros past the count
    assert len(guards.unwritten(d_gt)) == 0
    guards.check()
    # the compact form: a plain batch, no index list
    guards.repoison(d_gt); guards.repoison(d_cnt)
    _crop_gt(ctx, guards.inp(gt[index]), guards.inp(cnt[index], dtype=np.int32), b, None, win, d_gt, d_cnt, b, gmax, h, w)
    np.testing.assert_array_equal(d_cnt.download(), [len(r) for r in rows])
    np.testing.assert_array_equal(d_gt.download(), want)
    # more rows than one wave: groups of 64 keep their order too
    big = np.concatenate([gt[0], gt[0, ::-1], gt[0, :2]])[None]
    rows = D._crop_gt([big[0]], win[:1], h, w)
    d_gt, d_cnt = guards.out((1, 130, 5)), guards.out((1,), np.int32)
    _crop_gt(ctx, guards.inp(big), guards.inp(np.array([130], np.int32), dtype=np.int32), 1, None, win[:1], d_gt, d_cnt, 1, 130, h, w)
    assert d_cnt.download().tolist() == [len(rows[0])] == [65]
    np.testing.assert_array_equal(d_gt.download()[0, :65], rows[0])
    assert not d_gt.download()[0, 65:].any()


def test_crop_rejects_bad_arguments_before_anything_is_written(ctx, guards):
    from ssdseglib import _hip as H
    b, h, w, gmax = 2, 4, 8, 3
    p_img, p_idx = guards.inp(np.zeros((N_POOL, h, w, 3), np.uint8)), guards.inp(np.zeros((N_POOL, h, w), np.uint8))
    p_gt, p_cnt = guards.inp(np.zeros((N_POOL, gmax, 5), np.float32)), guards.inp(np.ones(N_POOL, np.int32), dtype=np.int32)
    d_img, d_idx, d_flip = guards.out((b, h, w, 3), np.uint8), guards.out((b, h, w), np.uint8), guards.out((b,), np.uint8)
    d_gt, d_cnt = guards.out((b, gmax, 5)), guards.out((b,), np.int32)
    good_index, good = [1, 0], [(0, 0, w, h), (1, 1, 4, 2)]
    nan = float("nan")
    cases = [   # (index, second window, the argument the error names in crop_inputs / crop_gt)
        ([0, N_POOL], good[1], 5), ([-1, 0], good[1], 5),
        (good_index, (0, nan, 4, 2), 6), (good_index, (0, 0, float("inf"), 2), 6),
        (good_index, (0, 0, 0.5, 2), 6), (good_index, (0, 0, 4, 16 * h + 1), 6),
        (good_index, (17 * w, 0, 4, 2), 6), (good_index, (0, -17 * h, 4, 2), 6),
    ]
    for index, second, arg in cases:
        win = [good[0], second]
        with pytest.raises(H.SsdsegError, match=f"ssdseg_crop_inputs: invalid argument {arg} "):
            _crop_inputs(ctx, p_img, p_idx, N_POOL, index, win, FILL, 0, d_img, d_idx, b, h, w, flip=[1, 0], d_flip=d_flip)
        with pytest.raises(H.SsdsegError, match=f"ssdseg_crop_gt: invalid argument {arg} "):
            _crop_gt(ctx, p_gt, p_cnt, N_POOL, index, win, d_gt, d_cnt, b, gmax, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 8 "):
        _crop_inputs(ctx, p_img, p_idx, N_POOL, good_index, good, FILL, 256, d_img, d_idx, b, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 2 "):
        _crop_inputs(ctx, None, None, N_POOL, good_index, good, FILL, 0, d_img, d_idx, b, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 11 "):
        _crop_inputs(ctx, p_img, p_idx, N_POOL, good_index, good, FILL, 0, None, d_idx, b, h, w)
    with pytest.raises(H.SsdsegError, match="invalid argument 5 "):
        _crop_inputs(ctx, p_img, p_idx, 1, None, good, FILL, 0, d_img, d_idx, b, h, w)         # n -> n needs b source samples
    with pytest.raises(H.SsdsegError, match="invalid argument 7 "):
        _crop_gt(ctx, p_gt, p_cnt, N_POOL, good_index, good, None, d_cnt, b, gmax, h, w)
    ctx.sync()
    guards.check()
    for buf in (d_img, d_idx, d_flip, d_gt, d_cnt):          # nothing was launched: every output still holds the poison
        assert len(guards.unwritten(buf)) == buf.size, buf.alloc.name


# ---------------------------------------------------------------- the loaders and fit, on the small model
H_, W_ = SHAPE[:2]
WINDOWS = np.array([(10.25, 5.5, 64, 48), (0, 0, W_, H_), (-32, -12, 1.5 * W_, 1.25 * H_)], np.float32)      # zoom-in, identity, zoom-out
PICK = [4, 0, 2]


def _filled(eng, loader, batch):
    from ssdseglib._loaders import loader_for
    ld = loader_for(eng, batch)
    assert type(ld) is loader
    ld.stage(batch)
    ld.consume()
    return _buffers(eng)


def test_cropped_batches_fill_the_step_buffers_alike(ctx, guards, rng):
    """a ResidentBatch with windows == its compact copy == a plain CompactBatch cropped on the host by the spec (same flips and
    draws, no windows): crop, then flip, then colour -- for every combination of flips and colour draws"""
    import ssdseglib
    from ssdseglib import datacoder as D, _engine as E, _loaders as LD
    E.set_default_context(ctx)
    ds, cb = _resident(rng, 5)
    _, _, model = build(seed=5)
    _compile(model)
    eng = E.engine_for(model, 3, True)
    fill = FILL + (FILL_CLASS,)
    for flip, draws in (([1, 0, 1], None), ([0, 1, 1], _f32(HIGH)), (None, _f32(HIGH)), (None, None)):
        rb = ds.batch(PICK, flip, draws, crop_windows=WINDOWS, crop_fill=fill)
        compact = ds.to_compact(rb)
        assert np.array_equal(compact.crop_windows, WINDOWS) and compact.crop_fill == fill and compact.rgb_draws == rb.rgb_draws
        assert compact.images.tobytes() == cb.images[PICK].tobytes()                        # the copy holds the UNcropped samples
        img, idx = D._crop_resample(cb.images[PICK], cb.mask_index[PICK], WINDOWS, FILL, FILL_CLASS)
        gts = D._crop_gt([cb.ground_truth[s] for s in PICK], WINDOWS, H_, W_)
        assert img[1].tobytes() == cb.images[PICK[1]].tobytes() and np.array_equal(gts[1], cb.ground_truth[PICK[1]])      # the identity
        assert img[0].tobytes() != cb.images[PICK[0]].tobytes() and (idx[2] == FILL_CLASS).any()
        host = ssdseglib.datacoder.CompactBatch(img, idx, gts, compact.flip, cb.encoder, rgb_draws=draws)
        got = _filled(eng, LD._ResidentLoader, rb)
        same = _filled(eng, LD._CompactLoader, compact)
        want = _filled(eng, LD._CompactLoader, host)
        assert want["__input__"].any()
        for name in want:
            assert got[name].tobytes() == want[name].tobytes(), ("resident", name, flip, draws)
            assert same[name].tobytes() == want[name].tobytes(), ("compact", name, flip, draws)
    # all-identity windows: the bytes of the batch without windows
    ident = np.tile(np.array([0, 0, W_, H_], np.float32), (3, 1))
    flip, draws = [0, 1, 1], _f32(HIGH)
    plain = _filled(eng, LD._ResidentLoader, ds.batch(PICK, flip, draws))
    for loader, batch in ((LD._ResidentLoader, ds.batch(PICK, flip, draws, crop_windows=ident, crop_fill=fill)),
                          (LD._CompactLoader, ds.to_compact(ds.batch(PICK, flip, draws, crop_windows=ident)))):
        got = _filled(eng, loader, batch)
        for name in plain:
            assert got[name].tobytes() == plain[name].tobytes(), name
    # and a batch without windows after one with: the loader is back on its old path
    again = _filled(eng, LD._ResidentLoader, ds.batch(PICK, flip, draws))
    assert all(again[name].tobytes() == plain[name].tobytes() for name in plain)
    # train_on_batch takes the same objects
    rb = ds.batch([3, 1, 4], [1, 0, 0], _f32(HIGH), crop_windows=WINDOWS, crop_fill=fill)
    logs = model.train_on_batch(rb)
    _, _, model2 = build(seed=5)
    _compile(model2)
    assert logs == model2.train_on_batch(ds.to_compact(rb))


def _weights(model):
    return [w for layer in model.layers for w in layer.get_weights()]


CROP = dict(probability=0.7, scale=(0.5, 1.6), fill=FILL, fill_class=0)


def test_fit_on_a_cropping_resident_dataset_equals_fit_on_its_compact_batches(ctx, guards):
    """7 samples in batches of 3, 3, 1, flips, colour and crops on, two epochs, with a cropping validation set: the history and the
    final weights of fit(ds) are those of fit over the recorded compact copies (windows attached) of the same batches"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    plans, train = _recorded(1993, 7, seed=11, rgb_augmentation=True, random_crop=CROP)
    _, val = _recorded(7, 4, seed=3, random_crop=CROP)
    windows = np.concatenate([rb.crop_windows for plan in plans for rb in plan])
    identity = (windows == np.array([0, 0, W_, H_], np.float32)).all(axis=1)
    assert identity.any() and not identity.all() and all(cb.crop_windows is not None and cb.crop_fill == FILL + (0,) for ep in train for cb in ep)
    _, _, model = build(seed=5)
    _compile(model)
    want = model.fit(_Replay(train), epochs=2, validation_data=_Replay(val), verbose=0).history
    want_weights = _weights(model)
    ds, _ = _resident(np.random.default_rng(1993), 7, seed=11, rgb_augmentation=True, random_crop=CROP)
    vds, _ = _resident(np.random.default_rng(7), 4, seed=3, random_crop=CROP)
    _, _, model = build(seed=5)
    _compile(model)
    got = model.fit(ds, epochs=2, validation_data=vds, verbose=0).history
    assert len(want["loss"]) == 2 and "val_loss" in want and got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    got_weights = _weights(model)
    assert len(got_weights) == len(want_weights) > 100
    for a, b in zip(got_weights, want_weights):
        assert a.tobytes() == b.tobytes()
    # the crops matter: the same fit without them gives another history
    plain, _ = _resident(np.random.default_rng(1993), 7, seed=11, rgb_augmentation=True)
    _, _, model = build(seed=5)
    _compile(model)
    assert model.fit(plain, epochs=1, verbose=0).history["loss"][0] != want["loss"][0]


def test_evaluate_on_device_refuses_a_cropped_batch(ctx, guards, rng):
    import ssdseglib
    from ssdseglib import _engine as E, _fit
    E.set_default_context(ctx)
    ds, _ = _resident(rng, 3, flip=False)
    _, builder, model = build(seed=5)
    inference = builder.get_model_for_inference(model_trained=model, boxes_iou_threshold=0.5, labels_probability_threshold=0.5,
                                                use_segmentation_suppression=False, max_number_of_boxes_per_class=8,
                                                max_number_of_boxes_per_sample=20, suppress_background_boxes=False)
    rb = ds.batch([0, 1, 2], crop_windows=WINDOWS)
    for data in ([rb], [ds.to_compact(rb)], iter([rb])):
        with pytest.raises(ValueError, match="crop windows"):
            ssdseglib.evaluators.evaluate_on_device(inference, data, [0, 1, 2, 3], 0, [0.5])
    with pytest.raises(ValueError, match="crop windows"):
        _fit.run_evaluate(inference, rb, [(0.5, 0.5)])                  # the engine's own door is shut too
