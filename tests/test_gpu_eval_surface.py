"""What a user reads at the end of a run, against the fp64 oracle: the `val_*` values of `fit(validation_data=...)`, the history's
own arithmetic, the `losses.*` callables called directly, and `predict` (background suppression, batching).

Validation (A): after every `fit` call the device's current parameters and moving statistics are loaded into the fp64 oracle, which
then evaluates the validation batches with `training=False`: the three losses and the three metrics, size-weighted over a 2 + 1
pair of batches, against every `val_*` entry (1e-3 relative for the losses, 2e-4 * max(1, |v|) for the metrics: the bounds of
test_full_train_step_parity and test_metrics_inside_train_step_and_fit).  The evaluation engine is built in the first call and
reused by the later ones (asserted), after Adam at LR = 1e-2 has moved the weights.  Controls inside the test: the same oracle
quantities at the weights from BEFORE the call (what a stale transposed or zero-padded weight copy, or a stale bucket, would give)
and with `training=True` (batch statistics) on the current weights must MISS the bound; the miss ratios |device - control| / bound
are printed.  The moving statistics start as the batch statistics of the training images, perturbed per channel (mean by
N(0, 0.2) standard deviations, variance by U(0.5, 1.5)): both modes differ from the start, and the network stays in its working
range (with the moving statistics drawn around 0 / 1 regardless of the activations the ReLU6s saturate and the heads' outputs no
longer depend on the image).

Measured miss ratios on one MI355X (|device - control| / bound; > 1 is a miss.  Asserted in every call for val_loss, the mask
loss and the confidence loss with the weights before the call, and for val_loss with batch statistics):
                                    weights before the call                          batch statistics
                                    val_loss  mask loss  confidence  boxes loss      val_loss
    cross_entropy, call 1             2318.7     2335.5        89.8         6.8        1275.5
    cross_entropy, call 2              303.5      304.2        16.6         4.4         189.2
    cross_entropy, call 3              433.7      435.2        87.4        77.2        1302.4
    dice, call 1                       178.3      158.3       162.3       215.9         402.0
    dice_square, call 1                187.7      104.3       141.0       260.3         447.6
The three metrics miss too (ratios 23 to 1086 before the call, 7 to 1245 with batch statistics) with one exception, which is
therefore "not sensitivity-controlled": val_output-boxes_jaccard_iou_bounding_boxes_metric in cross_entropy call 2, ratio 0.0
against the weights before the call -- the few positive anchors' offsets sit at the ReLU6 bounds (quirk Q3) before and after
those two steps, so the decoded boxes are the same.  The boxes loss and the metrics are printed, not asserted.
test_validation_writes_no_state's control: a training engine's forward changes 100 % of the state bucket.

Wall time on one MI355X: about 4 s for the whole file (pytest: 3.8 s), the three-call validation test 1.0 s."""

import numpy as np
import pytest

from oracle import np_ops as O
from oracle.np_model import NpModel
from tests.test_gpu_full_model import CW, SHAPE, STDS, build, make_targets
from tests.test_gpu_head_ops import make_det_case
from tests.test_gpu_training_steps import LR, oracle_from_device, randomise_bn, snapshot
from _guard import poisoned_ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _ctx_poison(poisoned_ctx):
    """every activation, statistics table, workspace region and fresh allocation starts as NaN (tests/_guard.py)"""
    return poisoned_ctx


LW = (0.0, 1 / 3, 1 / 3, 1 / 3)
LOSS_TOL, METRIC_TOL = 1e-3, 2e-4
LOSS_KEYS = {"mask": "output-mask_loss", "conf": "output-labels_loss", "loc": "output-boxes_loss"}


# ---------------------------------------------------------------------------------------------------------------- helpers
def anchors_cxywh(boxes):
    return [boxes.get_boxes_coordinates_center_x('ssd'), boxes.get_boxes_coordinates_center_y('ssd'),
            boxes.get_boxes_coordinates_width('ssd'), boxes.get_boxes_coordinates_height('ssd')]


def compile_model(model, boxes, mask_loss="cross_entropy", lr=LR):
    import ssdseglib
    model.compile(optimizer=ssdseglib.optimizers.Adam(learning_rate=lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7),
                  loss={'output-mask': getattr(ssdseglib.losses, mask_loss)(classes_weights=CW), 'output-labels': ssdseglib.losses.confidence_loss,
                        'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights={'output-mask': 1.0, 'output-labels': 1.0, 'output-boxes': 1.0},
                  metrics={'output-mask': ssdseglib.metrics.jaccard_iou_segmentation_masks(classes_weights=CW),
                           'output-labels': ssdseglib.metrics.categorical_accuracy(classes_weights=LW),
                           'output-boxes': ssdseglib.metrics.jaccard_iou_bounding_boxes(*anchors_cxywh(boxes), STDS)})


def metric_keys(model):
    return {name: f"{name}_{fn.__name__}" for name, fn in model._compiled["metrics"].items()}


def perturbed_moving_statistics(model, rng, x):
    """moving statistics of a 'trained' state: the batch statistics of `x` (float32 oracle), perturbed per channel"""
    ref = NpModel(model, dtype=np.float32)
    ref.forward(x, training=True)
    for l in model.layers:
        if type(l).__name__ == "BatchNormalization":
            mean = np.asarray(ref.cache[l.name]["mean"], np.float64).reshape(-1)
            var = np.asarray(ref.cache[l.name]["var"], np.float64).reshape(-1)
            l.weights["moving_mean"] = (mean + rng.normal(0, 0.2, mean.size) * np.sqrt(var + 1e-3)).astype(np.float32)
            l.weights["moving_variance"] = (var * rng.uniform(0.5, 1.5, var.size)).astype(np.float32)


def make_batches(rng, boxes, sizes):
    out = []
    for n in sizes:
        _, _, targets = make_targets(rng, boxes, n)
        out.append((rng.integers(0, 256, (n,) + SHAPE).astype(np.float32), targets))
    return out


def oracle_logs(ref, boxes, batches, mkeys, mask_loss="cross_entropy", training=False):
    """the Keras-named logs of an evaluation pass over `batches` by the fp64 oracle: per batch the mean over its samples, over the
    batches the size-weighted mean"""
    sums, seen = {}, 0
    cw = np.asarray(CW, np.float64)
    for x, t in batches:
        n = x.shape[0]
        p_mask, p_labels, p_boxes = ref.forward(x, training=training)
        y_mask, y_labels, y_boxes = (np.asarray(t[k], np.float64) for k in ('output-mask', 'output-labels', 'output-boxes'))
        if mask_loss == "cross_entropy":
            l_mask, _ = O.cross_entropy_loss(y_mask, p_mask, cw)
        else:
            l_mask = O.dice_loss(y_mask, p_mask, cw, squared=mask_loss == "dice_square")
        l_conf, _, _ = O.confidence_loss(y_labels, p_labels)
        l_loc, _ = O.localization_loss(y_boxes, p_boxes)
        logs = {LOSS_KEYS["mask"]: l_mask.mean(), LOSS_KEYS["conf"]: l_conf.mean(), LOSS_KEYS["loc"]: l_loc.mean()}
        logs["loss"] = l_mask.mean() + l_conf.mean() + l_loc.mean()
        logs[mkeys['output-mask']] = O.metric_mask_iou(y_mask, p_mask, CW).mean()
        logs[mkeys['output-labels']] = O.metric_label_accuracy(y_labels, p_labels, LW).mean()
        logs[mkeys['output-boxes']] = O.metric_box_iou(y_boxes, p_boxes, *anchors_cxywh(boxes), STDS).mean()
        for k, v in logs.items():
            sums[k] = sums.get(k, 0.0) + float(v) * n
        seen += n
    return {"val_" + k: v / seen for k, v in sums.items()}


def bound(key, want):
    return LOSS_TOL * abs(want) if key.endswith("loss") else METRIC_TOL * max(1.0, abs(want))


def assert_logs(got, want, what):
    """every key of `want` in `got`, within its bound; NaN agrees with NaN (quirk Q10)"""
    for k, w in want.items():
        assert k in got, (what, k, sorted(got))
        g = got[k]
        print(f"  {what} {k}: device {g!r} oracle {w!r}")
        if np.isnan(w) or np.isnan(g):
            assert np.isnan(w) and np.isnan(g), (what, k, g, w)
        else:
            assert abs(g - w) < bound(k, w), (what, k, g, w, abs(g - w) / bound(k, w))


def miss_ratios(got, control):
    """|device - control| / bound(control) per key: > 1 means the control misses the bound the real comparison holds"""
    return {k: (abs(got[k] - c) / bound(k, c) if np.isfinite(c) and np.isfinite(got[k]) and bound(k, c) > 0 else float("nan"))
            for k, c in control.items()}


CONTROLLED = ("val_loss", "val_" + LOSS_KEYS["mask"], "val_" + LOSS_KEYS["conf"])


def fit_and_check(model, boxes, train, val, mask_loss, calls, tag):
    """`calls` separate fit(train, epochs=1, validation_data=val) calls, each judged from the state the device is in afterwards"""
    from ssdseglib import _engine as E
    mkeys = metric_keys(model)
    probe = E.engine_for(model, train[0][0].shape[0], True)         # (owns the shared buckets; the oracle reads them through it)
    assert (2, "eval") not in model.__dict__.get("_engines", {}), "the evaluation engines are created by fit"
    before = oracle_logs(oracle_from_device(model, probe), boxes, val, mkeys, mask_loss)
    evals = None
    for call in range(1, calls + 1):
        hist = model.fit(train, epochs=1, validation_data=val, verbose=0).history
        engines = {n: model._engines[(n, "eval")] for n in (2, 1)}
        if evals is None:
            evals = engines
        assert all(engines[n] is evals[n] for n in evals), "the evaluation engine of the first call is reused"
        assert all(e.P is probe.P and not e.training for e in evals.values())
        got = {k: v[0] for k, v in hist.items() if k.startswith("val_")}
        assert all(len(v) == 1 for v in hist.values())
        ref = oracle_from_device(model, probe)
        want = oracle_logs(ref, boxes, val, mkeys, mask_loss)
        assert set(want) == set(got), (sorted(want), sorted(got))
        assert_logs(got, want, f"{tag} call {call}")
        stale = miss_ratios(got, before)
        batch_stats = miss_ratios(got, oracle_logs(ref, boxes, val, mkeys, mask_loss, training=True))
        print(f"{tag} call {call}: miss ratios of the weights before the call {({k: round(v, 1) for k, v in stale.items()})}")
        print(f"{tag} call {call}: miss ratios of batch statistics {({k: round(v, 1) for k, v in batch_stats.items()})}")
        for k in CONTROLLED:
            assert stale[k] > 1, f"{tag} call {call}: stale-weights control of {k} does not miss its bound (ratio {stale[k]:.2f})"
        assert batch_stats["val_loss"] > 1, f"{tag} call {call}: batch-statistics control does not miss (ratio {batch_stats['val_loss']:.2f})"
        before = want


# ------------------------------------------------------------------------------------------------------- A. validation values
@pytest.mark.parametrize("mask_loss,calls", [("cross_entropy", 3), ("dice", 1), ("dice_square", 1)])
def test_validation_values_against_the_oracle(ctx, rng, mask_loss, calls):
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    randomise_bn(model, rng)
    train = make_batches(rng, boxes, (2, 1))
    val = make_batches(rng, boxes, (2, 1))
    perturbed_moving_statistics(model, rng, np.concatenate([x for x, _ in train]))
    compile_model(model, boxes, mask_loss)
    fit_and_check(model, boxes, train, val, mask_loss, calls, mask_loss)


def test_validation_of_compact_batches(ctx, rng):
    """validation_data as datacoder.CompactBatch (un-augmented): the oracle's targets are the evaluation engine's own, downloaded
    after the hand-over (the device encoder is pinned by test_encode_targets_exact), its images the uint8 pixels as floats"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    randomise_bn(model, rng)
    train = make_batches(rng, boxes, (2, 1))
    perturbed_moving_statistics(model, rng, np.concatenate([x for x, _ in train]))
    compile_model(model, boxes)
    val = []
    for n in (2, 1):
        enc, gts, targets = make_targets(rng, boxes, n)
        img = rng.integers(0, 256, (n,) + SHAPE).astype(np.uint8)
        val.append(ssdseglib.datacoder.CompactBatch(img, targets['output-mask'].argmax(-1).astype(np.uint8), gts, np.zeros(n, np.uint8), enc))
    hist = model.fit(train, epochs=1, validation_data=val, verbose=0).history
    probe = E.engine_for(model, 2, True)
    batches = []
    for cb in val:
        eng = model._engines[(len(cb), "eval")]
        ops = {kind: op for _, op, kind in eng._loss_names}
        t = {'output-mask': ops["mask"].y_true.download(), 'output-labels': ops["conf"].y_labels.download(), 'output-boxes': ops["loc"].y_boxes.download()}
        assert np.array_equal(t['output-mask'].argmax(-1), cb.mask_index) and t['output-labels'][..., 1:].sum() > 0
        assert np.array_equal(eng.input_store.buf.download().reshape(cb.images.shape), cb.images.astype(np.float32))
        batches.append((cb.images.astype(np.float32), t))
    want = oracle_logs(oracle_from_device(model, probe), boxes, batches, metric_keys(model))
    got = {k: v[0] for k, v in hist.items() if k.startswith("val_")}
    assert set(want) == set(got)
    assert_logs(got, want, "compact")


def test_validation_writes_no_state(ctx, rng):
    """the validation path alone (both batch sizes) leaves params, state, both Adam moments and the step counter bit-identical, and
    the training step after it gives the bits of the same step replayed from the snapshot without a validation in between.
    Control: a TRAINING engine's forward on the same batch does change `state` (the comparison can fail)."""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    randomise_bn(model, rng)
    compile_model(model, boxes)
    (x3, t3), = make_batches(rng, boxes, (3,))
    val = make_batches(rng, boxes, (2, 1))
    eng = E.engine_for(model, 3, True)
    opt = model._compiled["optimizer"]
    eng.train_step(x3, t3, optimizer=opt)             # non-trivial moments, counter and moving statistics
    s0 = snapshot(ctx, eng)
    assert s0["t"] == 1 and np.abs(s0["m"]).max() > 0

    def same(a, b):
        return a["t"] == b["t"] and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in "psmv")

    def validate():
        for x, t in val:
            ev = E.eval_engine_for(model, x.shape[0])
            ev.set_input(x)
            ev.set_targets(t)
            ev.forward()
            ev.compute_metrics()
            logs = ev.losses()
            assert all(np.isfinite(v) for k, v in logs.items() if "loss" in k), logs

    def step():
        eng.train_step(x3, t3, optimizer=opt)
        return snapshot(ctx, eng), eng.P["grads"].download(), eng.losses()

    validate()
    validate()                                       # the second pass reuses the engines
    assert same(snapshot(ctx, eng), s0), "validation changed params, state, Adam moments or the step counter"
    after_val = step()
    P = eng.P
    P["params"].upload(s0["p"]); P["state"].upload(s0["s"]); eng.opt.slot("m").upload(s0["m"]); eng.opt.slot("v").upload(s0["v"]); eng.opt.step = s0["t"]
    replay = step()
    assert same(after_val[0], replay[0]) and np.array_equal(after_val[1].view(np.uint32), replay[1].view(np.uint32))
    assert after_val[2].keys() == replay[2].keys() and all(after_val[2][k] == replay[2][k] or np.isnan(replay[2][k]) for k in replay[2])
    assert after_val[0]["t"] == 2 and not same(after_val[0], s0)
    # control
    s1 = snapshot(ctx, eng)
    eng.set_input(val[0][0][:1].repeat(3, axis=0))
    eng.forward()
    ctx.join()
    s2 = snapshot(ctx, eng)
    changed = float((s1["s"] != s2["s"]).mean())
    print(f"control: a training forward changes {changed:.0%} of the state bucket")
    assert changed > 0.5 and np.array_equal(s1["p"], s2["p"])


# ------------------------------------------------------------------------------------------------ B. training-history arithmetic
def test_fit_history_is_the_size_weighted_mean_of_train_on_batch(ctx, rng):
    """fit's per-epoch logs over a ragged 2 + 1 pair of batches == sum(v * n) / sum(n) of train_on_batch's logs in the same order, to
    1e-12 relative: a handful of double operations on the same float32 batch means (the kernels are deterministic)"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, _ = build()
    train = make_batches(rng, boxes, (2, 1))
    models = []
    for _ in range(2):
        _, _, model = build()
        randomise_bn(model, np.random.default_rng(7))
        compile_model(model, boxes)
        models.append(model)
    epochs = 2
    hist = models[0].fit(train, epochs=epochs, verbose=0).history
    want = {}
    for _ in range(epochs):
        sums, seen = {}, 0
        for x, t in train:
            n = x.shape[0]
            for k, v in models[1].train_on_batch(x, t).items():
                sums[k] = sums.get(k, 0.0) + v * n
            seen += n
        for k, v in sums.items():
            want.setdefault(k, []).append(v / seen)
    assert set(hist) == set(want) and {"loss", *LOSS_KEYS.values(), *metric_keys(models[0]).values()} == set(hist)
    for k in want:
        assert len(hist[k]) == epochs
        for g, w in zip(hist[k], want[k]):
            assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= 1e-12 * abs(w), (k, hist[k], want[k])
    assert hist["loss"][1] != hist["loss"][0] and all(np.isfinite(hist[k]).all() for k in ("loss", *LOSS_KEYS.values()))


# ----------------------------------------------------------------------------------------------- C. standalone loss callables
def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


MASK_SHAPES = [(2, 6, 8, 4), (3, 120, 160, 4),           # one block; 10 blocks and the grid-stride loop
               (1, 1, 1, 4), (1, 384, 352, 4)]           # one pixel; 135,168 pixels > 64 * 2048: the block count saturates at 64


def mask_case(rng, shape):
    """probabilities and one-hot targets (float32); from 8 pixels up: true-class probabilities of exactly 0, 1, 5e-8 and 1 - 5e-8
    (the clip of the cross-entropy runs), an exact one-hot row, and a pixel with no class set"""
    n, h, w, c = shape
    p = O.softmax(rng.normal(0, 2, shape)).astype(np.float32)
    cls = rng.integers(0, c, shape[:3])
    y = np.eye(c, dtype=np.float32)[cls]
    if h * w >= 8:
        pf, yf, cf = p.reshape(n, h * w, c), y.reshape(n, h * w, c), cls.reshape(n, h * w)
        for i, v in enumerate(np.array([0.0, 1.0, 5e-8, 1.0 - 5e-8], np.float32)):
            for b in range(n):
                pf[b, i] = (1 - v) / 3
                pf[b, i, cf[b, i]] = v
        yf[0, 5] = 0                                    # no class set: the formulas are on values, not on an arg-max
        pf[-1, 6] = yf[-1, 6]                           # an exact one-hot prediction
    return y, p


@pytest.mark.parametrize("shape", MASK_SHAPES)
def test_standalone_mask_losses(ctx, rng, shape):
    """losses.cross_entropy(w) (the `squared == 2` branch of the dice kernels), dice(w), dice_square(w) called directly"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    y, p = mask_case(rng, shape)
    y64, p64, cw = y.astype(np.float64), p.astype(np.float64), np.asarray(CW, np.float64)
    want_ce, _ = O.cross_entropy_loss(y64, p64, cw)
    got_ce = ssdseglib.losses.cross_entropy(CW)(y, p)
    assert got_ce.shape == (shape[0],) and rel(got_ce, want_ce) < 1e-5, (got_ce, want_ce)
    if shape[1] * shape[2] >= 8:
        assert want_ce.min() > -np.log(1e-7) * min(CW)  # the clipped pixels weigh in: log(0) unclipped would be inf
    for name, squared in (("dice", False), ("dice_square", True)):
        got = getattr(ssdseglib.losses, name)(CW)(y, p)
        assert got.shape == (shape[0],) and rel(got, O.dice_loss(y64, p64, cw, squared=squared)) < 1e-5, name


def det_cases(rng):
    for b, a, pos_frac in [(4, 600, 0.03), (2, 9600, 0.01), (3, 500, 0.0), (2, 300, 0.6)]:            # those of test_det_loss
        yield (f"random {b}x{a} {pos_frac}",) + make_det_case(rng, b, a, pos_frac)
    y, p, yb, pb = make_det_case(rng, 2, 400, 0.5)
    cls = rng.integers(1, 4, (2, 400))
    yield "no background anchor", np.eye(4, dtype=np.float32)[cls], p, (rng.normal(0, 2, (2, 400, 4))).astype(np.float32), pb
    y, p, yb, pb = make_det_case(rng, 2, 400, 0.5)
    cls[1] = 0
    yb = (rng.normal(0, 2, (2, 400, 4)) * (cls > 0)[..., None]).astype(np.float32)
    yield "all positive | none", np.eye(4, dtype=np.float32)[cls], p, yb, pb


def test_standalone_detection_losses(ctx, rng):
    """losses.confidence_loss / localization_loss called directly (one loss output, every other output NULL, dummy inputs for the
    other half) against the oracle on the same float32 inputs"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    for name, y, p, yb, pb in det_cases(rng):
        conf_ref, _, keep = O.confidence_loss(y, p)
        loc_ref, _ = O.localization_loss(yb, pb)
        conf = ssdseglib.losses.confidence_loss(y, p)
        loc = ssdseglib.losses.localization_loss(yb, pb)
        assert conf.shape == loc.shape == (y.shape[0],), name
        n_bg, n_pos = int((y[..., 0] == 1).sum()), int((y[..., 0] == 0).sum())
        assert keep.sum() == min(3 * n_pos, n_bg), name
        for got, want, what in ((conf, conf_ref, "confidence"), (loc, loc_ref, "localization")):
            if np.abs(want).max() == 0:
                assert not got.any(), (name, what, got)
            else:
                assert rel(got, want) < 1e-5, (name, what, got, want)
        if name == "all positive | none":
            assert loc[1] == 0 and loc_ref[1] == 0 and conf_ref[1] > 0      # image 1: no object, hard negatives only
        if name == "no background anchor":
            assert n_bg == 0 and keep.sum() == 0


# ---------------------------------------------------------------------------------------------------- E. inference surface
def inference_models(rng, batch_for_statistics=3):
    boxes, builder, model = build(seed=5)
    randomise_bn(model, rng)
    x = rng.integers(0, 256, (19,) + SHAPE).astype(np.float32)
    perturbed_moving_statistics(model, rng, x[:batch_for_statistics])
    kw = dict(model_trained=model, max_number_of_boxes_per_class=4, max_number_of_boxes_per_sample=10, boxes_iou_threshold=0.3,
              labels_probability_threshold=0.4, use_segmentation_suppression=True)
    return builder, x, builder.get_model_for_inference(suppress_background_boxes=False, **kw), builder.get_model_for_inference(suppress_background_boxes=True, **kw)


def test_suppress_background_boxes(ctx, rng):
    """quirk Q7: suppress_background_boxes=True flattens the detections, drops label 0 and loses the batch axis == the
    suppress_background_boxes=False output filtered in NumPy, bit for bit; both == the oracle tail on the device's head tensors"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    _, x, keep_bg, drop_bg = inference_models(rng)
    x = x[:3]
    seg, det = keep_bg.predict([x])
    seg2, det2 = drop_bg.predict([x])
    assert det.shape == (3, 10, 6) and det2.ndim == 2 and det2.shape[1] == 6
    flat = det.reshape(-1, 6)
    n_bg, n_fg = int((flat[:, 0] == 0).sum()), int((flat[:, 0] > 0).sum())
    assert n_bg > 0 and n_fg > 0, (n_bg, n_fg)
    assert det2.shape[0] == n_fg and np.array_equal(det2.view(np.uint32), flat[flat[:, 0] > 0].view(np.uint32))
    assert np.array_equal(seg.view(np.uint32), seg2.view(np.uint32))
    eng = E.engine_for(keep_bg, 3, False)
    eng.set_input(x); eng.forward()
    probs = eng.vals[id(keep_bg.get_layer('output-labels').outputs[0])].store.buf.download().reshape(3, -1, 4)
    offs = eng.vals[id(keep_bg.get_layer('output-boxes').outputs[0])].store.buf.download().reshape(3, -1, 4)
    dec = keep_bg.get_layer('decode-output-boxes')
    cent = np.stack([dec.center_x_boxes_default, dec.center_y_boxes_default, dec.width_boxes_default, dec.height_boxes_default], axis=1)
    want, valid = O.combined_nms(O.decode_to_corners_pred(offs, cent, STDS), O.seg_suppress(eng.output(0), probs), 4, 10, 0.3, 0.4)
    wflat = want.reshape(-1, 6)
    assert valid.min() > 0 and ((wflat[:, 0] == 0) & (wflat[:, 1] > 0.4)).any(), "real background detections, not only padding"
    assert np.array_equal(det[..., 0], want[..., 0]) and np.abs(det - want).max() < 1e-3
    wflat = wflat[wflat[:, 0] > 0]
    assert np.array_equal(det2[:, 0], wflat[:, 0]) and np.abs(det2 - wflat).max() < 1e-3


def test_predict_batching(ctx, rng):
    """predict on a (19, H, W, 3) array (chunks of 16 + 3: two engines) == predict on the two chunks == 19 single-image calls"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    _, x, model, _ = inference_models(rng)
    seg_a, det_a = model.predict(x)
    assert seg_a.shape == (19,) + SHAPE[:2] + (4,) and det_a.shape == (19, 10, 6)
    assert {(16, False), (3, False)} <= set(model._engines)
    seg_b, det_b = model.predict([x[:16], x[16:]])
    singles = [model.predict([x[i:i + 1]]) for i in range(19)]
    seg_c, det_c = np.concatenate([s for s, _ in singles]), np.concatenate([d for _, d in singles])
    assert len({d.tobytes() for d in det_a}) == 19, "the detections should depend on the image"
    print("predict batching: max |mask| difference array vs chunks", np.abs(seg_a - seg_b).max(), "array vs singles", np.abs(seg_a - seg_c).max(),
          "detection rows that differ (chunks, singles)", int((det_a != det_b).any(-1).sum()), int((det_a != det_c).any(-1).sum()))
    assert np.array_equal(det_a.view(np.uint32), det_b.view(np.uint32)) and np.array_equal(seg_a.view(np.uint32), seg_b.view(np.uint32))
    assert np.array_equal(det_a.view(np.uint32), det_c.view(np.uint32))
    assert np.array_equal(seg_a.view(np.uint32), seg_c.view(np.uint32))
