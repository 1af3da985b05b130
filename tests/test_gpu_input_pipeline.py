"""GPU parity of the input side of the step: a compact batch -- uint8 pixels, uint8 class indices, ground-truth
rows, flip flags -- expanded on the device (csrc/inputs.hip + ssdseg_encode_targets) vs the oracle's restatement of
DataEncoderDecoder.read_and_encode (reference datacoder.py:302-347).  Byte / index work -- pixels, one-hot rows, mirrored boxes,
matched labels -- is bit-exact; the encoded offsets hold a float32 log (datacoder.py:268-269) and are compared at 1e-5 like
tests/test_gpu_head_ops.py::test_encode_targets_exact."""
import numpy as np
import pytest

from oracle import np_ops as O
from tests.test_gpu_full_model import CW, SHAPE, build, make_targets
from _guard import BODY_WORD, guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("b,h,w,c,with_flip", [(3, 7, 13, 4, True), (2, 9, 16, 3, True), (1, 5, 5, 8, False), (4, 48, 64, 4, True)])
def test_expand_inputs_bit_exact(ctx, guards, rng, b, h, w, c, with_flip):
    img = rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, c + 2, (b, h, w)).astype(np.uint8)         # c, c+1: out of range -> all-zero one-hot rows
    flip = (np.arange(b) % 2 == 0).astype(np.uint8) if with_flip else None
    want_img, want_mask = O.expand_inputs(img, idx, flip, c)
    d_img, d_mask = guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    d_flip = guards.inp(flip, dtype=np.uint8) if flip is not None else None
    ctx.call("ssdseg_expand_inputs", guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8), d_flip, d_img, d_mask,
             b, h, w, c)
    np.testing.assert_array_equal(d_img.download(), want_img)
    np.testing.assert_array_equal(d_mask.download(), want_mask)
    # either half alone
    guards.check()
    guards.repoison(d_img); guards.repoison(d_mask)
    ctx.call("ssdseg_expand_inputs", guards.inp(img, dtype=np.uint8), None, d_flip, d_img, None, b, h, w, c)
    ctx.call("ssdseg_expand_inputs", None, guards.inp(idx, dtype=np.uint8), d_flip, None, d_mask, b, h, w, c)
    np.testing.assert_array_equal(d_img.download(), want_img)
    np.testing.assert_array_equal(d_mask.download(), want_mask)


B_BLOCKS = 130                          # two full 64-sample kernel-argument blocks (csrc/batch_sel.h) and two samples
BLOCK_SHAPES = [(2, 8, 4), (2, 8, 3), (3, 5, 4), (3, 5, 3)]      # (h, w, c): four pixels per thread in the colour kernels / one; float4 one-hot rows / loops


def _block_flags(rng):
    """flip flags of B_BLOCKS samples that differ across both block edges"""
    flip = rng.integers(0, 2, B_BLOCKS).astype(np.uint8)
    flip[[63, 64, 127, 128]] = [1, 0, 0, 1]
    return flip


@pytest.mark.parametrize("h,w,c", BLOCK_SHAPES)
def test_expand_inputs_of_130_samples(ctx, guards, rng, h, w, c):
    """a plain batch has no 64-sample block: more samples than one block holds, flags from the device array"""
    b = B_BLOCKS
    img = rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, c + 2, (b, h, w)).astype(np.uint8)
    flip = _block_flags(rng)
    want_img, want_mask = O.expand_inputs(img, idx, flip, c)
    d_img, d_mask = guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    ctx.call("ssdseg_expand_inputs", guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8), guards.inp(flip, dtype=np.uint8), d_img, d_mask,
             b, h, w, c)
    np.testing.assert_array_equal(d_img.download(), want_img)
    np.testing.assert_array_equal(d_mask.download(), want_mask)
    guards.check()


PLACEMENTS = ["image source", "class-index source", "image destination", "one-hot destination"]
ODD_SHAPE = (2, 3, 8, 4)                # (b, h, w, c): the width allows four pixels per thread, c a float4 per one-hot row; a shifted buffer does not


class Shifted:
    """the buffers of one call with ONE of them off its alignment: a uint8 source one byte, or a float destination one float,
    into a guarded allocation (dword loads / float4 stores there would fault or hit the wrong bytes).  `b`: the sources are
    pools, the outputs a batch of b; idx / c None: the call takes no class indices."""

    def __init__(self, guards, img, idx, which, b=None, c=None):
        assert which in PLACEMENTS
        shape = (len(img) if b is None else b,) + img.shape[1:]
        self.img = self._source(guards, img, which == "image source")
        self.idx = self._source(guards, idx, which == "class-index source") if idx is not None else None
        self._img_whole, self.out = self._destination(guards, shape, which == "image destination")
        if c is not None:
            self._mask_whole, self.mask_out = self._destination(guards, shape[:3] + (c,), which == "one-hot destination")

    @staticmethod
    def _source(guards, a, shifted):
        if not shifted:
            return guards.inp(a, dtype=np.uint8)
        return guards.inp(np.concatenate([[0], a.ravel(), [0] * 7]), dtype=np.uint8).view(1, a.shape)

    @staticmethod
    def _destination(guards, shape, shifted):
        """(the allocation a shifted view lies in or None, the buffer to hand to the call)"""
        if not shifted:
            return None, guards.out(shape)
        whole = guards.out((int(np.prod(shape)) + 4,))
        return whole, whole.view(1, shape)

    @staticmethod
    def _body(whole, out):
        """what the call wrote; around a shifted destination the poison must be intact"""
        if whole is None:
            return out.download()
        raw, n = whole.download(), out.size
        assert (np.concatenate([raw[:1], raw[1 + n:]]).view(np.uint32) == BODY_WORD).all()
        return raw[1:1 + n].reshape(out.shape)

    def image(self):
        return self._body(self._img_whole, self.out)

    def mask(self):
        return self._body(self._mask_whole, self.mask_out)

    def repoison(self, guards):
        for whole, out in ((self._img_whole, self.out), (getattr(self, "_mask_whole", None), getattr(self, "mask_out", None))):
            if out is not None:
                guards.repoison(whole if whole is not None else out)


@pytest.mark.parametrize("which", PLACEMENTS)
def test_expand_inputs_falls_back_on_a_misaligned_buffer(ctx, guards, rng, which):
    b, h, w, c = ODD_SHAPE
    img = rng.integers(0, 256, (b, h, w, 3)).astype(np.uint8)
    idx = rng.integers(0, c + 2, (b, h, w)).astype(np.uint8)
    flip = np.array([1, 0], np.uint8)
    want_img, want_mask = O.expand_inputs(img, idx, flip, c)
    d_flip = guards.inp(flip, dtype=np.uint8)
    a_img, a_mask = guards.out((b, h, w, 3)), guards.out((b, h, w, c))
    ctx.call("ssdseg_expand_inputs", guards.inp(img, dtype=np.uint8), guards.inp(idx, dtype=np.uint8), d_flip, a_img, a_mask, b, h, w, c)
    s = Shifted(guards, img, idx, which, c=c)
    ctx.call("ssdseg_expand_inputs", s.img, s.idx, d_flip, s.out, s.mask_out, b, h, w, c)
    assert s.image().tobytes() == a_img.download().tobytes() == want_img.tobytes()
    assert s.mask().tobytes() == a_mask.download().tobytes() == want_mask.tobytes()
    guards.check()


def test_expand_inputs_rejects_bad_arguments(ctx, guards):
    from ssdseglib import _hip as H
    buf = guards.out((1, 2, 2, 3))
    u8 = guards.out((1, 2, 2, 3), np.uint8)
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_expand_inputs", None, None, None, buf, None, 1, 2, 2, 4)       # nothing to expand
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_expand_inputs", u8, None, None, None, None, 1, 2, 2, 4)        # no destination
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_expand_inputs", u8, None, None, buf, None, 1, 2, 2, 9)         # more classes than the kernel's row


def test_flip_gt_boxes_bit_exact(ctx, guards, rng):
    b, gmax, width = 5, 6, 640.0
    gt = np.zeros((b, gmax, 5), np.float32)
    cnt = rng.integers(0, gmax + 1, b).astype(np.int32)
    cnt[0] = gmax
    for n in range(b):
        x0 = rng.uniform(0, 500, cnt[n]); x1 = x0 + rng.uniform(1, 139, cnt[n])
        gt[n, :cnt[n]] = np.stack([rng.integers(1, 4, cnt[n]), x0, rng.uniform(0, 400, cnt[n]), x1, rng.uniform(400, 479, cnt[n])], axis=1)
    gt[:, :, 0][gt[:, :, 0] == 0] = 0
    flip = np.array([1, 0, 1, 1, 0], np.uint8)
    want = gt.copy()
    for n in range(b):
        if flip[n]:
            want[n, :cnt[n]] = O.flip_gt_boxes(gt[n, :cnt[n]], width)
    d = guards.out(gt.shape).upload(gt)     # flipped in place
    ctx.call("ssdseg_flip_gt_boxes", d, guards.inp(cnt, dtype=np.int32), guards.inp(flip, dtype=np.uint8), b, gmax, width)
    np.testing.assert_array_equal(d.download(), want)       # rows past the count and unflagged samples untouched


def test_flip_gt_boxes_of_130_samples(ctx, guards, rng):
    b, gmax, width = B_BLOCKS, 4, 640.0
    cnt = rng.integers(0, gmax + 1, b).astype(np.int32)
    cnt[[63, 64, 127, 128]] = gmax
    gt = np.zeros((b, gmax, 5), np.float32)
    for n in range(b):
        x0 = rng.uniform(0, 500, cnt[n]); x1 = x0 + rng.uniform(1, 139, cnt[n])
        gt[n, :cnt[n]] = np.stack([rng.integers(1, 4, cnt[n]), x0, rng.uniform(0, 400, cnt[n]), x1, rng.uniform(400, 479, cnt[n])], axis=1)
    flip = _block_flags(rng)
    want = gt.copy()
    for n in range(b):
        if flip[n]:
            want[n, :cnt[n]] = O.flip_gt_boxes(gt[n, :cnt[n]], width)
    d = guards.out(gt.shape).upload(gt)     # flipped in place
    ctx.call("ssdseg_flip_gt_boxes", d, guards.inp(cnt, dtype=np.int32), guards.inp(flip, dtype=np.uint8), b, gmax, width)
    np.testing.assert_array_equal(d.download(), want)


def _compile(model):
    import ssdseglib
    model.compile(optimizer=ssdseglib.optimizers.Adam(learning_rate=1e-3),
                  loss={'output-mask': ssdseglib.losses.cross_entropy(classes_weights=CW), 'output-labels': ssdseglib.losses.confidence_loss,
                        'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights={'output-mask': 1.0, 'output-labels': 1.0, 'output-boxes': 1.0})


def _compact_batches(rng, sizes):
    """compact batches and, beside them, the float tensors the reference's map would hand over for the same samples, from the
    ORACLE (expand + flip + encode_targets restated in NumPy)"""
    import ssdseglib
    out = []
    for bsz in sizes:
        boxes, _, _ = build()
        enc, gts, targets = make_targets(rng, boxes, bsz)
        idx = targets['output-mask'].argmax(-1).astype(np.uint8)
        img = rng.integers(0, 256, (bsz,) + SHAPE).astype(np.uint8)
        flip = rng.integers(0, 2, bsz).astype(np.uint8)
        flip[0] = 1
        cb = ssdseglib.datacoder.CompactBatch(img, idx, gts, flip, enc)
        want_img, want_mask = O.expand_inputs(img, idx, flip, 4)
        corners = np.stack([enc.xmin_boxes_default, enc.ymin_boxes_default, enc.xmax_boxes_default, enc.ymax_boxes_default], axis=1).astype(np.float32)
        labels, offsets = [], []
        for g, f in zip(gts, flip):
            g = O.flip_gt_boxes(g, SHAPE[1]) if f else g
            l, o, _ = O.encode_targets(corners, g, 4, 0.525, enc._stds)
            labels.append(l); offsets.append(o)
        out.append((cb, want_img, {'output-mask': want_mask, 'output-labels': np.stack(labels), 'output-boxes': np.stack(offsets)}))
    return out


def _device_encoded(cb, targets):
    """the same float targets with the offsets from the DEVICE encoder on the oracle-mirrored boxes (the float32 log inside
    differs from NumPy's by an ulp now and then; a bit-for-bit comparison of two fits needs identical inputs)"""
    gts = [O.flip_gt_boxes(g, SHAPE[1]) if f else g for g, f in zip(cb.ground_truth, cb.flip)]
    labels, offsets = cb.encoder.encode_batch(gts)
    np.testing.assert_array_equal(labels, targets['output-labels'])
    return dict(targets, **{'output-boxes': offsets})


def test_compact_batch_fills_the_step_buffers_like_the_oracle(ctx, guards, rng):
    """the engine's input / mask / label / offset buffers after a compact hand-over == the oracle's float tensors, bit for bit"""
    from ssdseglib import _engine as E, _loaders as LD
    E.set_default_context(ctx)
    (cb, want_img, want), = _compact_batches(rng, (3,))
    _, _, model = build(seed=5)
    _compile(model)
    eng = E.engine_for(model, 3, True)
    ld = LD.loader_for(eng, cb)
    assert type(ld) is LD._CompactLoader
    ld.stage(cb)
    ld.consume()
    np.testing.assert_array_equal(eng.input_store.buf.download().reshape(want_img.shape), want_img)
    for name, op, kind in eng._loss_names:
        got = (op.y_true if kind == "mask" else (op.y_labels if kind == "conf" else op.y_boxes)).download()
        if kind == "loc":
            assert np.abs(got.reshape(want[name].shape) - want[name]).max() < 1e-5      # float32 log of the size ratio
        else:
            np.testing.assert_array_equal(got.reshape(want[name].shape), want[name], err_msg=name)


def test_fit_on_compact_batches_equals_fit_on_float_tensors(ctx, guards, rng, monkeypatch):
    """model.fit over compact batches (uploads overlapped with the running step, and synchronous) gives the history of the
    same fit over the expanded float32 tensors -- identical device kernels on identical inputs, so identical bits; a smaller
    last batch goes through another engine"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    data = [(cb, img, _device_encoded(cb, t)) for cb, img, t in _compact_batches(rng, (3, 3, 3, 2))]
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
    # train_on_batch takes the same object
    _, _, model = build(seed=5)
    _compile(model)
    logs = model.train_on_batch(data[0][0])
    _, _, model2 = build(seed=5)
    _compile(model2)
    assert logs == model2.train_on_batch(data[0][1], data[0][2])


def test_compact_batch_errors(ctx, rng):
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    (cb, _, _), = _compact_batches(rng, (2,))
    with pytest.raises(ValueError):
        ssdseglib.datacoder.CompactBatch(cb.images, cb.mask_index[:, :-1], cb.ground_truth, cb.flip, cb.encoder)
    with pytest.raises(ValueError):
        ssdseglib.datacoder.CompactBatch(cb.images, cb.mask_index, cb.ground_truth[:1], cb.flip, cb.encoder)
    _, _, model = build(seed=5)
    _compile(model)
    crowded = ssdseglib.datacoder.CompactBatch(cb.images, cb.mask_index, [np.tile(cb.ground_truth[0][:1], (65, 1)), cb.ground_truth[1]], cb.flip, cb.encoder)
    with pytest.raises(ValueError, match="64"):
        model.train_on_batch(crowded)
    # an encoder built for another class count than the model's heads: the encode kernel would overrun / mis-stride the target
    # buffers -- refused when the loader is made
    import copy
    enc5 = copy.copy(cb.encoder)
    enc5.num_classes = 5
    wrong = ssdseglib.datacoder.CompactBatch(cb.images, cb.mask_index, cb.ground_truth, cb.flip, enc5)
    _, _, model2 = build(seed=5)
    _compile(model2)
    with pytest.raises(ValueError, match="num_classes"):
        model2.train_on_batch(wrong)
