"""fit's look-ahead across kinds of batch (ssdseglib/_fit.py run_fit, _loaders.loader_for / loader_ahead): one epoch over dense,
compact (two encoder objects), resident and one-sample batches, with the look-ahead on and off, against train_on_batch batch by
batch.  The same kernels see the same bytes in the same order either way, so histories and final weights are compared for equality."""
import numpy as np
import pytest

from tests.test_gpu_full_model import build
from tests.test_gpu_input_pipeline import _compact_batches, _compile, _device_encoded
from tests.test_gpu_resident_dataset import _resident
from _guard import guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _weights(model):
    return [w for layer in model.layers for w in layer.get_weights()]


@pytest.fixture()
def went_ahead(monkeypatch):
    """(loader class name, accepted) of every stage(..., ahead=True) call, in order"""
    from ssdseglib import _loaders as LD
    log = []

    def spy(cls, inner):
        def stage(self, x, y=None, ahead=False):
            went = inner(self, x, y, ahead)
            if ahead:
                log.append((cls.__name__, went))
            return went
        monkeypatch.setattr(cls, "stage", stage)
    for cls in (LD._DenseLoader, LD._CompactLoader, LD._ResidentLoader):
        spy(cls, cls.stage)
    return log


def _fit(batches, overlap, went_ahead, monkeypatch):
    """-> history, final weights and what went ahead of one fit(epochs=1) of a fresh model"""
    monkeypatch.delenv("SSDSEG_FIT_OVERLAP", raising=False)
    if not overlap:
        monkeypatch.setenv("SSDSEG_FIT_OVERLAP", "0")
    _, _, model = build(seed=5)
    _compile(model)
    del went_ahead[:]
    hist = model.fit(batches, epochs=1, verbose=0).history
    return hist, _weights(model), list(went_ahead)


def test_fit_hands_over_between_loader_kinds_like_train_on_batch(ctx, guards, rng, monkeypatch, went_ahead):
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    (a, a_img, a_t), (b, b_img, b_t), (c, _, _), (d, _, _), (e, _, _), (one, _, _) = _compact_batches(rng, (3, 3, 3, 3, 3, 1))
    first, second = c.encoder, e.encoder
    assert first is not second and first.num_classes == second.num_classes

    def with_first(cb):
        return ssdseglib.datacoder.CompactBatch(cb.images, cb.mask_index, cb.ground_truth, cb.flip, first)
    ds, _ = _resident(rng, 5)
    batches = [(a_img, _device_encoded(a, a_t)), (b_img, _device_encoded(b, b_t)),     # dense, dense
               c, with_first(d), e,                                                    # compact: first, first, second encoder
               ds.batch([4, 0, 2], [1, 0, 1]),                                         # resident
               with_first(one),                                                        # compact, 1 sample: another engine
               (b_img, _device_encoded(b, b_t))]                                       # dense
    want, want_w, staged = _fit(batches, True, went_ahead, monkeypatch)
    # what went ahead: the second dense batch under the first, the second compact batch of the first encoder under the first
    assert staged == [("_DenseLoader", True), ("_CompactLoader", True)]
    got, got_w, staged = _fit(batches, False, went_ahead, monkeypatch)
    assert staged == []
    _, _, twin = build(seed=5)
    _compile(twin)
    sums, seen = {}, 0
    for item in batches:
        x, y = item if isinstance(item, tuple) else (item, None)
        n = len(x)
        for k, v in twin.train_on_batch(x, y).items():
            sums[k] = sums.get(k, 0.0) + v * n
        seen += n
    assert seen == 22 and set(want) == set(got) == set(sums) and "loss" in want
    for k in want:
        assert want[k] == got[k] == [sums[k] / seen], k
    twin_w = _weights(twin)
    assert len(want_w) == len(got_w) == len(twin_w) > 100
    for w0, w1, w2 in zip(want_w, got_w, twin_w):
        assert w0.tobytes() == w1.tobytes() == w2.tobytes()


def test_a_dense_batch_goes_ahead_under_a_compact_or_resident_step(ctx, guards, rng, monkeypatch, went_ahead):
    """a dense batch of the same size is staged under whatever step runs; one without host arrays for every target is declined and
    goes the synchronous way"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    (a, a_img, a_t), (b, b_img, b_t), (c, _, _) = _compact_batches(rng, (3, 3, 3))
    ds, _ = _resident(rng, 5)
    y_a, y_b = _device_encoded(a, a_t), _device_encoded(b, b_t)
    on_device = dict(y_b, **{'output-boxes': ctx.array(y_b['output-boxes'])})
    batches = [c, (a_img, y_a), ds.batch([1, 3, 0], [0, 1, 1]), (b_img, y_b), c, (b_img, on_device)]
    want, want_w, staged = _fit(batches, True, went_ahead, monkeypatch)
    assert staged == [("_DenseLoader", True), ("_DenseLoader", True), ("_DenseLoader", False)]
    got, got_w, staged = _fit(batches, False, went_ahead, monkeypatch)
    assert staged == [] and set(want) == set(got) and "loss" in want
    for k in want:
        assert want[k] == got[k], k
    assert len(want_w) == len(got_w) > 100
    for w0, w1 in zip(want_w, got_w):
        assert w0.tobytes() == w1.tobytes()


def test_the_doors_that_take_no_loader_shortcuts(ctx, guards, rng):
    """the engine's own evaluate door refuses flips and colour draws (the class indices it compares with are never mirrored), and
    a dense validation batch without targets is an error, not a forward pass against the targets of the batch before"""
    from ssdseglib import _engine as E, _fit
    E.set_default_context(ctx)
    (a, a_img, a_t), = _compact_batches(rng, (3,))
    ds, _ = _resident(rng, 3, flip=False)
    _, builder, model = build(seed=5)
    inference = builder.get_model_for_inference(model_trained=model, boxes_iou_threshold=0.5, labels_probability_threshold=0.5,
                                                use_segmentation_suppression=False, max_number_of_boxes_per_class=8,
                                                max_number_of_boxes_per_sample=20, suppress_background_boxes=False)
    assert a.flip.any()
    for batch in (a, ds.batch([0, 1, 2], [0, 1, 0]), ds.batch([0, 1, 2], None, (0.1, 1.1, 1.1, 0.1))):
        with pytest.raises(ValueError, match="not augmented"):
            _fit.run_evaluate(inference, batch, [(0.5, 0.5)])
    iou, _ = _fit.run_evaluate(inference, ds.batch([0, 1, 2], [0, 0, 0]), [(0.5, 0.5)])       # flags that flip nothing are fine
    assert iou.shape == (3, 4)
    _compile(model)
    with pytest.raises(ValueError, match="targets"):
        model.fit([(a_img, _device_encoded(a, a_t))], epochs=1, validation_data=[a_img], verbose=0)
