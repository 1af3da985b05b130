"""The colour augmentation of the reference's input pipeline (DataEncoderDecoder.augmentation_rgb_channels, reference
datacoder.py:434-466) on compact batches: the draws travel with the CompactBatch, ssdseg_rgb_augment (csrc/inputs.hip) applies
them on the GPU while the batch is expanded.  The host spec is datacoder._augment_rgb (itself checked against colorsys in
tests/test_cpu_cabi_and_host.py); the kernel follows it operation for operation, so the two agree to float32 rounding (2e-3 on
the 0..255 scale, the bound the host function meets against colorsys)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_input_pipeline import (B_BLOCKS, BLOCK_SHAPES, ODD_SHAPE, PLACEMENTS, Shifted, _block_flags, _compact_batches, _compile,
                                           _device_encoded)
from tests.test_gpu_full_model import build
from _guard import guards  # noqa: F401  (fixture)

LOW = (-0.05, 0.95, 0.90, -0.10)        # the low end of every reference range (datacoder.py:452-461)
HIGH = (0.05, 1.05, 1.10, 0.10)         # the high end
IDENTITY = (0.0, 1.0, 1.0, 0.0)
CLAMP = (0.5, 3.0, 2.5, 40.0)           # out of range: saturation and the final [0, 255] clip both clamp
ATOL = 2e-3


# ---------------------------------------------------------------------------------------------- host side (no GPU)
def _tiny_compact(draws=None):
    from ssdseglib import datacoder as D
    img = np.arange(2 * 3 * 4 * 3, dtype=np.uint8).reshape(2, 3, 4, 3)
    return D.CompactBatch(img, np.zeros((2, 3, 4), np.uint8), [np.zeros((0, 5), np.float32)] * 2, np.array([1, 0], np.uint8), None,
                          rgb_draws=draws)


def test_augmentation_of_a_compact_batch_attaches_draws(monkeypatch):
    from ssdseglib import datacoder as D
    cb = _tiny_compact()
    targets = {"output-mask": object()}
    out, t = D.augmentation_rgb_channels(cb, targets)
    assert t is targets
    assert isinstance(out, D.CompactBatch) and out is not cb
    assert cb.rgb_draws is None                                        # the input batch is left alone
    assert out.images is cb.images and out.mask_index is cb.mask_index and out.encoder is cb.encoder     # shared, not copied
    assert np.shares_memory(out.flip, cb.flip)
    assert all(np.array_equal(g, h) for g, h in zip(out.ground_truth, cb.ground_truth))
    hue, sat, con, bri = out.rgb_draws
    assert -0.05 <= hue <= 0.05 and 0.95 <= sat <= 1.05 and 0.90 <= con <= 1.10 and -0.10 <= bri <= 0.10
    # the compact branch consumes the same four numbers, in the same order, as the float branch
    monkeypatch.setattr(D, "_aug_rng", np.random.default_rng(7))
    compact_draws = D.augmentation_rgb_channels(cb, None)[0].rgb_draws
    seen = []
    monkeypatch.setattr(D, "_augment_rgb", lambda x, *d: seen.append(d) or x)
    monkeypatch.setattr(D, "_aug_rng", np.random.default_rng(7))
    D.augmentation_rgb_channels(np.zeros((1, 2, 2, 3), np.float32), None)
    assert seen == [compact_draws]


def test_compact_batch_rejects_bad_draws():
    from ssdseglib import datacoder as D
    assert _tiny_compact().rgb_draws is None
    assert _tiny_compact((0, 1, 1, 0)).rgb_draws == (0.0, 1.0, 1.0, 0.0)
    for bad in [(1, 2, 3), (1, 2, 3, 4, 5), (0.0, 1.0, float("nan"), 0.0), (0.0, float("inf"), 1.0, 0.0), "abcd", 3.0]:
        with pytest.raises(ValueError):
            _tiny_compact(bad)
    assert isinstance(_tiny_compact(np.array([0.01, 1.0, 1.0, 0.0], np.float32)), D.CompactBatch)


# ---------------------------------------------------------------------------------------------- GPU
def _pixels(rng, b, h, w):
    """random pixels with grey ones (r = g = b), two tied channels (each pair, as max and as min), 0 and 255"""
    img = rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8)
    f = img.reshape(-1, 3)
    k = rng.integers(0, 6, f.shape[0])
    f[k == 0] = f[k == 0][:, :1]
    f[k == 1, 1] = f[k == 1, 0]
    f[k == 2, 2] = f[k == 2, 1]
    f[k == 3, 0] = f[k == 3, 2]
    f[k == 4] = rng.choice(np.array([0, 255], np.uint8), (int((k == 4).sum()), 3))
    f[0], f[-1] = (0, 0, 0), (255, 255, 255)
    if f.shape[0] > 3:
        f[1], f[2] = (255, 0, 255), (40, 40, 200)
    return img


def _f32(draws):
    return tuple(float(np.float32(v)) for v in draws)


def _host(img, flip, draws):
    """-> (_augment_rgb mirrored where flagged, float64 means of the hue- and saturation-adjusted image, the float32 means
    _augment_rgb itself centres on)"""
    from ssdseglib import datacoder as D
    x = img.astype(np.float32)
    want = D._augment_rgb(x, *draws)
    hsv = D._rgb_to_hsv(x)                      # the first two steps of _augment_rgb
    hsv[..., 0] = (hsv[..., 0] + draws[0]) % 1.0
    hsv = D._rgb_to_hsv(D._hsv_to_rgb(hsv))
    hsv[..., 1] = np.clip(hsv[..., 1] * draws[1], 0.0, 1.0)
    q = D._hsv_to_rgb(hsv)
    if flip is not None:
        want[flip != 0] = want[flip != 0][:, :, ::-1]
    return want, q.astype(np.float64).mean(axis=(1, 2)), q.mean(axis=(1, 2))


def _device(ctx, guards, img, flip, draws):
    b, h, w, _ = img.shape
    means, out = guards.out((b, 3)), guards.out((b, h, w, 3))
    d_flip = guards.inp(flip, dtype=np.uint8) if flip is not None else None
    ctx.call("ssdseg_rgb_augment", guards.inp(img, dtype=np.uint8), d_flip, (C.c_float * 4)(*draws), means, out, b, h, w)
    return out.download(), means.download()


CASES = [(s, d) for s in [(3, 7, 13), (1, 5, 5), (2, 9, 16), (4, 48, 64)] for d in (LOW, HIGH, IDENTITY, CLAMP)] + \
        [((8, 480, 640), d) for d in (HIGH, CLAMP)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,draws", CASES)
def test_rgb_augment_matches_the_host_spec(ctx, guards, rng, shape, draws):
    draws = _f32(draws)
    img = _pixels(rng, *shape)
    want, m64, m32 = _host(img, None, draws)
    # _augment_rgb centres the contrast on a float32 NumPy mean (summation error up to ~1e-5 relative at 480x640); the kernel's
    # mean is reduced in double.  That difference moves the output by |1 - contrast| * |m32 - m64| and nothing else.
    tol = ATOL + abs(1.0 - draws[2]) * float(np.abs(m32 - m64).max())
    flip = (np.arange(shape[0]) % 2 == 0).astype(np.uint8)
    for f in (None, flip):
        got, means = _device(ctx, guards, img, f, draws)
        guards.check()
        np.testing.assert_allclose(means, m64, rtol=1e-5)
        w = want if f is None else np.where(f[:, None, None, None] != 0, want[:, :, ::-1], want)
        err = float(np.abs(got - w).max())
        assert err <= tol, (shape, draws, f is not None, err, tol)
        assert got.min() >= 0.0 and got.max() <= 255.0


def _tolerance(draws, m64, m32):
    """the bound of test_rgb_augment_matches_the_host_spec: ATOL plus what the float32 mean of the host spec moves the output"""
    return ATOL + abs(1.0 - draws[2]) * float(np.abs(m32 - m64).max())


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", sorted({s[:2] for s in BLOCK_SHAPES}))
def test_rgb_augment_of_130_samples(ctx, guards, rng, h, w):
    """a plain batch has no 64-sample block: more samples than one block holds, flags from the device array"""
    draws = _f32(HIGH)
    img = _pixels(rng, B_BLOCKS, h, w)
    flip = _block_flags(rng)
    want, m64, m32 = _host(img, flip, draws)
    got, means = _device(ctx, guards, img, flip, draws)
    guards.check()
    np.testing.assert_allclose(means, m64, rtol=1e-5)
    err = float(np.abs(got - want).max())
    assert err <= _tolerance(draws, m64, m32), (err, _tolerance(draws, m64, m32))


@pytest.mark.gpu
@pytest.mark.parametrize("which", [p for p in PLACEMENTS if p.startswith("image")])       # the call takes no class indices
def test_rgb_augment_falls_back_on_a_misaligned_buffer(ctx, guards, rng, which):
    b, h, w, _ = ODD_SHAPE
    draws = _f32(HIGH)
    img = _pixels(rng, b, h, w)
    flip = np.array([1, 0], np.uint8)
    want, m64, m32 = _host(img, flip, draws)
    a_img, a_means = _device(ctx, guards, img, flip, draws)
    s, means = Shifted(guards, img, None, which), guards.out((b, 3))
    ctx.call("ssdseg_rgb_augment", s.img, guards.inp(flip, dtype=np.uint8), (C.c_float * 4)(*draws), means, s.out, b, h, w)
    assert s.image().tobytes() == a_img.tobytes() and means.download().tobytes() == a_means.tobytes()
    guards.check()
    np.testing.assert_allclose(a_means, m64, rtol=1e-5)
    assert float(np.abs(a_img - want).max()) <= _tolerance(draws, m64, m32)


@pytest.mark.gpu
def test_rgb_augment_is_deterministic(ctx, guards, rng):
    img = _pixels(rng, 32, 480, 640)
    flip = rng.integers(0, 2, 32).astype(np.uint8)
    a, ma = _device(ctx, guards, img, flip, _f32(HIGH))
    b, mb = _device(ctx, guards, img, flip, _f32(HIGH))
    assert a.tobytes() == b.tobytes() and ma.tobytes() == mb.tobytes()


@pytest.mark.gpu
def test_rgb_augment_rejects_bad_arguments(ctx, guards):
    from ssdseglib import _hip as H
    u8, means, out = guards.out((1, 2, 4, 3), np.uint8), guards.out((1, 3)), guards.out((1, 2, 4, 3))
    draws = (C.c_float * 4)(*IDENTITY)
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_rgb_augment", None, None, draws, means, out, 1, 2, 4)
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_rgb_augment", u8, None, draws, None, out, 1, 2, 4)
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_rgb_augment", u8, None, (C.c_float * 4)(0.0, float("nan"), 1.0, 0.0), means, out, 1, 2, 4)
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_rgb_augment", u8, None, draws, means, out, 0, 2, 4)


def _augmented(cb, draws):
    from ssdseglib import datacoder as D
    return D.CompactBatch(cb.images, cb.mask_index, cb.ground_truth, cb.flip, cb.encoder, rgb_draws=_f32(draws))


def _target_buffers(eng):
    return {name: (op.y_true if kind == "mask" else (op.y_labels if kind == "conf" else op.y_boxes)).download()
            for name, op, kind in eng._loss_names}


@pytest.mark.gpu
def test_loader_augments_only_the_image(ctx, guards, rng):
    from ssdseglib import _engine as E, _loaders as LD
    E.set_default_context(ctx)
    (cb, _, _), = _compact_batches(rng, (3,))
    _, _, model = build(seed=5)
    _compile(model)
    eng = E.engine_for(model, 3, True)
    ld = LD.loader_for(eng, cb)
    assert type(ld) is LD._CompactLoader
    ld.stage(cb)
    ld.consume()
    plain = _target_buffers(eng)
    aug = _augmented(cb, HIGH)
    ld.stage(aug)
    ld.consume()
    want, _, _ = _host(cb.images, cb.flip, aug.rgb_draws)
    got = eng.input_store.buf.download().reshape(want.shape)
    assert float(np.abs(got - want).max()) <= ATOL
    for name, buf in _target_buffers(eng).items():
        assert buf.tobytes() == plain[name].tobytes(), name


def _augmented_data(ctx, guards, rng, sizes, draw_sets):
    """(augmented compact batch, the same batch as float tensors: the ssdseg_rgb_augment image downloaded, device-encoded targets)"""
    out = []
    for (cb, _, t), draws in zip(_compact_batches(rng, sizes), draw_sets):
        aug = _augmented(cb, draws)
        img, _ = _device(ctx, guards, cb.images, cb.flip, aug.rgb_draws)
        out.append((aug, img, _device_encoded(cb, t)))
    return out


@pytest.mark.gpu
def test_fit_on_augmented_compact_batches_equals_fit_on_float_tensors(ctx, guards, rng, monkeypatch):
    """fit over augmented compact batches -- uploads overlapped with the running step, and synchronous -- gives the history of
    the same fit over the augmented float32 tensors, bit for bit; a smaller last batch goes through another engine"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    data = _augmented_data(ctx, guards, rng, (3, 3, 3, 2), (LOW, HIGH, CLAMP, (0.02, 0.97, 1.04, -0.06)))
    hist = {}
    for mode in ("compact-overlap", "compact-sync", "float"):
        monkeypatch.setenv("SSDSEG_FIT_OVERLAP", "0" if mode == "compact-sync" else "1")
        _, _, model = build(seed=5)
        _compile(model)
        batches = [cb for cb, _, _ in data] if mode != "float" else [(img, t) for _, img, t in data]
        hist[mode] = model.fit(batches, epochs=2, verbose=0).history
    for mode in ("compact-overlap", "compact-sync"):
        assert hist[mode].keys() == hist["float"].keys()
        for k in hist["float"]:
            assert hist[mode][k] == hist["float"][k], (mode, k, hist[mode][k], hist["float"][k])


@pytest.mark.gpu
def test_fit_validates_on_compact_batches(ctx, guards, rng):
    """validation_data as compact batches (augmented or not) gives the val_* history of the same batches as float tensors"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    train = [cb for cb, _, _ in _augmented_data(ctx, guards, rng, (3, 3), (LOW, HIGH))]
    val = _augmented_data(ctx, guards, rng, (3, 2), (HIGH, IDENTITY))
    (plain_cb, plain_img, plain_t), = [(cb, img, _device_encoded(cb, t)) for cb, img, t in _compact_batches(rng, (3,))]
    hist = {}
    for mode in ("compact", "float"):
        _, _, model = build(seed=5)
        _compile(model)
        vdata = [cb for cb, _, _ in val] + [plain_cb] if mode == "compact" else [(img, t) for _, img, t in val] + [(plain_img, plain_t)]
        hist[mode] = model.fit(train, epochs=2, validation_data=vdata, verbose=0).history
    val_keys = [k for k in hist["float"] if k.startswith("val_")]
    assert "val_loss" in val_keys and hist["compact"].keys() == hist["float"].keys()
    for k in hist["float"]:
        assert hist["compact"][k] == hist["float"][k], (k, hist["compact"][k], hist["float"][k])
