"""GPU parity of the focal confidence loss (`ssdseg_det_loss_focal`) and of independent detection loss weights
(`ssdseg_det_loss_scaled`): the kernels against the fp64 oracle of tests/_focal_oracle.py (pinned by test_cpu_focal_oracle.py),
the localization half against `ssdseg_det_loss` bit for bit, and the engine / Keras surface on top.

Error bounds are test_det_loss's: loss rel_err < 1e-5, d_logits rel_err < 2e-5 (or both sides exactly zero),
|d_boxes - ref| < 1e-6.  The oracle gets the float32 probabilities, so it clips at the device's float32 constants."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import np_ops as O
from oracle.np_model import NpModel
import _focal_oracle as F
from _guard import guards  # noqa: F401  (fixture)
from tests.test_gpu_backbone import device_relu_masks, rel
from tests.test_gpu_full_model import CW, SHAPE, build, make_targets
from tests.test_gpu_head_ops import make_det_case, make_det_edge_case, rel_err, saturated_case

pytestmark = pytest.mark.gpu

GAMMAS = [0.0, 0.5, 2.0, 5.0]
ALPHAS = [(1.0, 1.0, 1.0, 1.0), (0.25, 1.0, 0.75, 0.5)]
CASES = [(4, 600, 0.03),      # ordinary case
         (3, 500, 0.0),       # no object anywhere: divide by 1, background gradient only
         (2, 300, 0.6),       # many positives
         (2, 300, 1.0),       # no background at all
         (1, 37, 0.1),        # fewer anchors than blocks per image: empty blocks, ragged chunk
         (2, 9600, 0.01)]     # the real anchor count
NAMES = ("conf", "loc", "dlog", "dbox")


@functools.lru_cache(maxsize=None)
def det_case(b, a, pos_frac):
    """one input set per shape, shared by every gamma / alpha (read-only)"""
    arrays = make_det_case(np.random.default_rng(1993), b, a, pos_frac)
    for v in arrays:
        v.setflags(write=False)
    return arrays


def c4(alpha):
    return (C.c_float * 4)(*alpha)


def references(y, p, yb, pb, alpha, gamma, conf_scale, loc_scale):
    conf_ref, dp_ref = F.focal_confidence_loss(y, p, alpha, gamma)
    loc_ref, dloc_ref = O.localization_loss(yb, pb)
    return dict(conf=conf_ref, loc=loc_ref, dlog=O.softmax_bwd(p.astype(np.float64), dp_ref) * conf_scale, dbox=dloc_ref * loc_scale)


def run_focal(ctx, guards, ins, shape, alpha, gamma, conf_scale, loc_scale, present=NAMES):
    b, a = shape
    shapes = dict(conf=(b,), loc=(b,), dlog=(b, a, 4), dbox=(b, a, 4))
    outs = {k: guards.out(shapes[k]) for k in present}
    ctx.call("ssdseg_det_loss_focal", *ins, b, a, 4, c4(alpha), gamma, conf_scale, loc_scale, *[outs.get(k) for k in NAMES])
    ctx.sync()
    guards.check()
    for k in present:
        assert guards.unwritten(outs[k]).size == 0, k
    return {k: outs[k].download() for k in present}


def assert_parity(got, ref, what=""):
    errs = {k: rel_err(got[k], ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(got[k]).max()) for k in ("conf", "loc", "dlog")}
    errs["dbox"] = float(np.abs(got["dbox"] - ref["dbox"]).max())
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(np.isfinite(v).all() for v in got.values())
    assert errs["conf"] < 1e-5 or (np.abs(ref["conf"]).max() == 0 and errs["conf"] == 0)
    assert errs["loc"] < 1e-5 or (np.abs(ref["loc"]).max() == 0 and errs["loc"] == 0)
    assert errs["dlog"] < 2e-5 or (np.abs(ref["dlog"]).max() == 0 and errs["dlog"] == 0)
    assert errs["dbox"] < 1e-6


# ------------------------------------------------------------------------------------------------ 1. kernel against the oracle
@pytest.mark.parametrize("b,a,pos_frac", CASES)
@pytest.mark.parametrize("alpha", ALPHAS, ids=["alpha1", "alphas"])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_focal_loss_parity(ctx, guards, gamma, alpha, b, a, pos_frac):
    y, p, yb, pb = det_case(b, a, pos_frac)
    conf_scale, loc_scale = 2.0 / b, 0.5 / b
    ins = [guards.inp(v) for v in (y, p, yb, pb)]
    got = run_focal(ctx, guards, ins, (b, a), alpha, gamma, conf_scale, loc_scale)
    ref = references(y, p, yb, pb, alpha, gamma, conf_scale, loc_scale)
    assert np.abs(ref["conf"]).max() > 0 and np.abs(ref["dlog"]).max() > 0
    if pos_frac == 0.0:
        assert not (y[..., 1:] != 0).any() and not ref["dbox"].any() and not got["dbox"].any()
    assert_parity(got, ref, f"gamma={gamma} alpha={alpha} {(b, a, pos_frac)}")


# -------------------------------------------------------------------------------------- 2. the localization half, bit for bit
def run_mined(ctx, guards, ins, shape, scales, entry):
    b, a = shape
    outs = dict(conf=guards.out(b), loc=guards.out(b), dlog=guards.out((b, a, 4)), dbox=guards.out((b, a, 4)), keep=guards.out(b * a, np.uint8))
    ctx.call(entry, *ins, b, a, 4, *scales, *[outs[k] for k in NAMES + ("keep",)])
    ctx.sync()
    guards.check()
    return {k: v.download() for k, v in outs.items()}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def test_localization_half_is_bit_identical_and_scales_are_independent(ctx, guards):
    b, a = 4, 600
    y, p, yb, pb = det_case(b, a, 0.03)
    ins = [guards.inp(v) for v in (y, p, yb, pb)]
    s = 1.0 / b
    mined = run_mined(ctx, guards, ins, (b, a), (s,), "ssdseg_det_loss")
    assert np.abs(mined["dbox"]).max() > 0 and mined["keep"].sum() > 0
    focal = run_focal(ctx, guards, ins, (b, a), ALPHAS[1], 2.0, 3.0 * s, s)
    assert np.array_equal(bits(focal["loc"]), bits(mined["loc"]))
    assert np.array_equal(bits(focal["dbox"]), bits(mined["dbox"]))
    same = run_mined(ctx, guards, ins, (b, a), (s, s), "ssdseg_det_loss_scaled")
    for k in NAMES + ("keep",):
        assert np.array_equal(bits(same[k]), bits(mined[k])), k
    # different scales: each gradient follows its own
    conf_scale, loc_scale = 2.0 / b, 0.5 / b
    got = run_mined(ctx, guards, ins, (b, a), (conf_scale, loc_scale), "ssdseg_det_loss_scaled")
    conf_ref, dp_ref, keep_ref = O.confidence_loss(y, p)
    loc_ref, dloc_ref = O.localization_loss(yb, pb)
    assert np.array_equal(got["keep"], keep_ref)
    ref = dict(conf=conf_ref, loc=loc_ref, dlog=O.softmax_bwd(p.astype(np.float64), dp_ref.astype(np.float64)) * conf_scale,
               dbox=dloc_ref * loc_scale)
    assert_parity(got, ref, "mined, two scales")
    assert np.array_equal(bits(got["conf"]), bits(mined["conf"])) and np.array_equal(bits(got["loc"]), bits(mined["loc"]))


# ---------------------------------------------------------------------------------------- 3. clip edges, saturated logits
@pytest.mark.parametrize("gamma", GAMMAS)
def test_focal_loss_clip_edges_and_saturated_logits(ctx, guards, rng, gamma):
    """Probabilities at exact 0 and 1 and at both float32 neighbours of each clip constant (make_det_edge_case), and softmax
    rows of logits from {0, 1.5, 6}.  A positive whose true-class probability is outside the clip range has an exactly zero
    gradient row.  A background anchor with p_bg = 1.0f has an exactly zero gradient row; its loss is what the definition's
    clip leaves, (2^-23)^gamma * 1.19e-7 per anchor (zero at the scale of the 1e-5 bound: below 5e-11 for gamma >= 0.5),
    checked on an image that holds nothing else."""
    alpha = ALPHAS[1]
    b, a = 2, 640
    y, p, yb, pb = make_det_edge_case(rng, b, a)
    conf_scale, loc_scale = 2.0 / b, 0.5 / b
    got = run_focal(ctx, guards, [guards.inp(v) for v in (y, p, yb, pb)], (b, a), alpha, gamma, conf_scale, loc_scale)
    ref = references(y, p, yb, pb, alpha, gamma, conf_scale, loc_scale)
    assert_parity(got, ref, f"edges gamma={gamma}")
    lo, hi = np.float32(1e-7), np.float32(1.0) - np.float32(1e-7)
    true_p = (p * y).sum(-1)
    outside = (true_p < lo) | (true_p > hi)
    dead = (y[..., 0] == 0) & outside
    assert dead.sum() >= 12 and not got["dlog"][dead].any()
    bg_one = (y[..., 0] == 1) & (p[..., 0] == 1.0)
    assert bg_one.sum() >= 1 and not got["dlog"][bg_one].any()
    live = (y[..., 0] == 0) & ~outside & (np.abs(ref["dlog"]).max(-1) > 1e-30)      # (above float32's denormal range)
    assert live.sum() >= 3 and got["dlog"][live].any(-1).all()

    # saturated heads: whole runs of equal rows
    b, a = 3, 1200
    ys, ps = saturated_case(rng, b, a, 0.05)
    zeros = np.zeros((b, a, 4), np.float32)
    got = run_focal(ctx, guards, [guards.inp(v) for v in (ys, ps, zeros, zeros)], (b, a), alpha, gamma, conf_scale, loc_scale)
    assert_parity(got, references(ys, ps, zeros, zeros, alpha, gamma, conf_scale, loc_scale), f"saturated gamma={gamma}")

    # an image of background anchors with p = (1, 0, 0, 0) only
    b, a = 1, 37
    y1 = np.tile(np.eye(4, dtype=np.float32)[0], (b, a, 1))
    zeros = np.zeros((b, a, 4), np.float32)
    got = run_focal(ctx, guards, [guards.inp(v) for v in (y1, y1, zeros, zeros)], (b, a), (1.0, 1.0, 1.0, 1.0), gamma, 1.0, 1.0)
    assert not got["dlog"].any()
    per_anchor = (2.0 ** -23) ** gamma * -np.log1p(-2.0 ** -23)
    assert abs(got["conf"][0] - a * per_anchor) <= max(1e-5 * a * per_anchor, a * 2.0 ** -126)   # (gamma = 5: a float32 denormal)
    if gamma > 0:
        assert got["conf"][0] < 37 * 5e-11


# ---------------------------------------------------------------------------------------------------- 4. optional outputs
def test_focal_loss_optional_outputs(ctx, guards):
    """the NULL subsets the product uses (training: all four; evaluation: the two losses; losses.focal_confidence_loss: conf
    alone): what is present is bit-identical to the full call, everything present is written, no guard is touched"""
    b, a = 3, 2400
    arrays = make_det_case(np.random.default_rng(5), b, a, 0.02)
    ins = [guards.inp(v) for v in arrays]
    full = run_focal(ctx, guards, ins, (b, a), ALPHAS[1], 2.0, 2.0 / b, 0.5 / b)
    assert np.abs(full["dlog"]).max() > 0 and np.abs(full["dbox"]).max() > 0
    for present in (("conf", "loc"), ("conf",)):
        part = run_focal(ctx, guards, ins, (b, a), ALPHAS[1], 2.0, 2.0 / b, 0.5 / b, present)
        for k in present:
            assert np.array_equal(bits(part[k]), bits(full[k])), (present, k)


def test_focal_loss_rejects_bad_arguments(ctx, guards):
    """bad gamma / alpha is an argument error of the call, before any launch"""
    from ssdseglib import _hip as H
    b, a = 1, 37
    ins = [guards.inp(v) for v in det_case(b, a, 0.1)]
    conf = guards.out(b)
    for alpha, gamma in (((1.0, 1.0, 1.0, 1.0), -1.0), ((1.0, 1.0, 1.0, 1.0), float("nan")), ((1.0, -1.0, 1.0, 1.0), 2.0),
                         ((1.0, 1.0, float("inf"), 1.0), 2.0)):
        with pytest.raises(H.SsdsegError):
            ctx.call("ssdseg_det_loss_focal", *ins, b, a, 4, c4(alpha), gamma, 1.0, 1.0, conf, None, None, None)
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_det_loss_focal", *ins, b, a, 3, c4(ALPHAS[0]), 2.0, 1.0, 1.0, conf, None, None, None)
    ctx.sync()
    assert guards.unwritten(conf).size == b


# --------------------------------------------------------------------------------------------------------- 5. determinism
def test_focal_loss_is_deterministic(ctx, guards):
    b, a = 2, 9600
    ins = [guards.inp(v) for v in det_case(b, a, 0.01)]
    first = run_focal(ctx, guards, ins, (b, a), ALPHAS[1], 2.0, 2.0 / b, 0.5 / b)
    second = run_focal(ctx, guards, ins, (b, a), ALPHAS[1], 2.0, 2.0 / b, 0.5 / b)
    for k in NAMES:
        assert np.array_equal(bits(first[k]), bits(second[k])), k


# ------------------------------------------------------------------------------------- 6. cross-check against the mined loss
def test_focal_gamma_zero_equals_the_mined_loss_when_mining_keeps_everything(ctx, guards):
    """pos_frac = 0.6 makes 3 P >= BG: mining keeps every background anchor, and gamma = 0, alpha = 1 is the same function.
    Device against device within 1e-5 relative (not bit-identical: the mined path takes the correctly rounded log)."""
    b, a = 2, 300
    y, p, yb, pb = det_case(b, a, 0.6)
    _, _, keep_ref = O.confidence_loss(y, p)
    assert np.array_equal(keep_ref.astype(bool), (y[..., 0] == 1).reshape(-1)) and keep_ref.sum() > 0
    ins = [guards.inp(v) for v in (y, p, yb, pb)]
    s = 1.0 / b
    mined = run_mined(ctx, guards, ins, (b, a), (s,), "ssdseg_det_loss")
    assert np.array_equal(mined["keep"], keep_ref)
    focal = run_focal(ctx, guards, ins, (b, a), ALPHAS[0], 0.0, s, s)
    assert rel_err(focal["conf"], mined["conf"]) < 1e-5
    assert rel_err(focal["dlog"], mined["dlog"]) < 1e-5
    assert np.array_equal(bits(focal["loc"]), bits(mined["loc"])) and np.array_equal(bits(focal["dbox"]), bits(mined["dbox"]))


# ------------------------------------------------------------------------------------------------------ engine-level tests
@pytest.fixture
def poison(ctx):
    """every activation, statistics table and workspace region of the engine starts as NaN (tests/_guard.py)"""
    ctx.debug_poison(True)
    try:
        yield ctx
    finally:
        ctx.debug_poison(False)


FOCAL_ALPHA, FOCAL_GAMMA = (0.25, 1.0, 0.75, 0.5), 2.0
WEIGHTS = {'output-mask': 1.0, 'output-labels': 2.0, 'output-boxes': 0.5}


def randomise_bn(model, rng):
    for l in model.layers:
        if type(l).__name__ == "BatchNormalization":
            c = l.weights["gamma"].size
            l.weights["gamma"] = rng.uniform(0.7, 1.3, c).astype(np.float32)
            l.weights["beta"] = rng.normal(0, 0.3, c).astype(np.float32)


def compile_det(model, conf_loss, weights, metrics=None):
    import ssdseglib
    model.compile(optimizer=ssdseglib.optimizers.Adam(learning_rate=1e-4),
                  loss={'output-mask': ssdseglib.losses.cross_entropy(classes_weights=CW), 'output-labels': conf_loss,
                        'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights=weights, metrics=metrics)


# -------------------------------------------------------------------------------------------------- 7. whole-step parity
@pytest.mark.parametrize("conf_kind", ["focal", "mined"])
def test_full_train_step_parity_with_unequal_detection_weights(ctx, poison, rng, conf_kind):
    """test_full_train_step_parity's set-up and bounds with loss_weights 1 / 2 / 0.5 and the focal (or the mined) confidence
    loss: outputs, the three losses, the weighted total and every parameter gradient against the fp64 oracle"""
    import ssdseglib
    from ssdseglib import _engine as E
    batch = 3
    boxes, builder, model = build()
    randomise_bn(model, rng)
    enc, gts, targets = make_targets(rng, boxes, batch)
    assert targets['output-labels'][..., 1:].sum() > 0, "test needs at least one positive anchor"
    conf_loss = ssdseglib.losses.focal_confidence_loss(FOCAL_ALPHA, FOCAL_GAMMA) if conf_kind == "focal" else ssdseglib.losses.confidence_loss
    compile_det(model, conf_loss, WEIGHTS)
    E.Engine.keep_mask_probabilities = True         # (so that output(0) can be compared)
    try:
        eng = E.Engine(model, batch, training=True, ctx=ctx)
    finally:
        E.Engine.keep_mask_probabilities = False
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    x = rng.integers(0, 256, (batch,) + SHAPE).astype(np.float32)

    ref = NpModel(model, dtype=np.float64)
    p_mask, p_labels, p_boxes = ref.forward(x, training=True)
    l_mask, dmask = O.cross_entropy_loss(targets['output-mask'].astype(np.float64), p_mask, np.asarray(CW, np.float64))
    y_labels = targets['output-labels'].astype(np.float64)
    if conf_kind == "focal":
        l_conf, dconf = F.focal_confidence_loss(y_labels, p_labels, FOCAL_ALPHA, FOCAL_GAMMA)
    else:
        l_conf, dconf, _ = O.confidence_loss(y_labels, p_labels)
    l_loc, dloc = O.localization_loss(targets['output-boxes'].astype(np.float64), p_boxes)
    w_mask, w_conf, w_loc = (WEIGHTS[k] for k in ('output-mask', 'output-labels', 'output-boxes'))

    eng.set_input(x)
    eng.set_targets(targets)
    eng.forward()
    assert np.abs(eng.output(0) - p_mask).max() < 2e-4
    assert np.abs(eng.output(1) - p_labels).max() < 2e-4
    assert rel(eng.output(2), p_boxes) < 1e-3
    got = eng.losses()
    assert abs(got['output-mask_loss'] - l_mask.mean()) < 1e-3 * abs(l_mask.mean())
    assert abs(got['output-labels_loss'] - l_conf.mean()) < 1e-3 * abs(l_conf.mean())
    assert abs(got['output-boxes_loss'] - l_loc.mean()) < 1e-3 * abs(l_loc.mean())
    total = w_mask * l_mask.mean() + w_conf * l_conf.mean() + w_loc * l_loc.mean()
    assert abs(got['loss'] - total) < 1e-3 * got['loss']
    weighted = w_mask * got['output-mask_loss'] + w_conf * got['output-labels_loss'] + w_loc * got['output-boxes_loss']
    assert abs(got['loss'] - weighted) <= 1e-12 * abs(weighted)

    eng.backward()
    ctx.sync()
    ref_grads = ref.backward([dmask * w_mask / batch, dconf * w_conf / batch, dloc * w_loc / batch], relu_masks=device_relu_masks(eng, model))
    worst, worst_name = 0.0, ""
    for l in model.layers:
        if not l.weights:
            continue
        scale = max(np.abs(ref_grads[l.name][w]).max() for w in l.trainable_names)
        if scale == 0:
            assert all(np.abs(eng.grad_view(l, w).download()).max() < 1e-12 for w in l.trainable_names), l.name
            continue
        for wname in l.trainable_names:
            g = eng.grad_view(l, wname).download()
            err = np.abs(g.astype(np.float64) - ref_grads[l.name][wname]).max() / scale
            if err > worst:
                worst, worst_name = err, f"{l.name}/{wname}"
            assert err < 1e-3, f"{l.name}/{wname}: rel err {err:.3e}"
    print("worst parameter-gradient rel err", worst, worst_name)


# -------------------------------------------------------------------------------------------------- 8. mined step untouched
def test_equal_weights_mined_step_is_the_single_scale_call(ctx, poison, rng, monkeypatch):
    """equal weights + confidence_loss: the engine still goes through `ssdseg_det_loss`, and the two-scale entry called by hand
    on the op's buffers leaves the same bits in logits.grad / boxes.grad, both losses and the whole gradient bucket"""
    import ssdseglib
    from ssdseglib import _engine as E
    batch = 3
    boxes, builder, model = build(seed=23)
    enc, gts, targets = make_targets(rng, boxes, batch)
    compile_det(model, ssdseglib.losses.confidence_loss, {'output-mask': 1.0, 'output-labels': 1.5, 'output-boxes': 1.5})
    eng = E.Engine(model, batch, training=True, ctx=ctx)
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    det = eng.loss_ops["det"]
    assert det.kind == "mined" and det.w_conf == det.w_loc == 1.5
    called = []
    real_call = ctx.call

    def spy(name, *args):
        called.append(name)
        return real_call(name, *args)

    x = rng.integers(0, 256, (batch,) + SHAPE).astype(np.float32)
    eng.set_input(x)
    eng.set_targets(targets)
    with monkeypatch.context() as m:
        m.setattr(ctx, "call", spy)
        eng.forward()
    assert "ssdseg_det_loss" in called and "ssdseg_det_loss_scaled" not in called and "ssdseg_det_loss_focal" not in called
    eng.backward()
    ctx.sync()
    want = [det.logits.grad.download(), det.boxes.grad.download(), det.conf_loss.download(), det.loc_loss.download(), eng.P["grads"].download()]
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0 and np.abs(want[4]).max() > 0

    eng.forward()
    for buf in (det.logits.grad, det.boxes.grad, det.conf_loss, det.loc_loss):
        buf.upload(np.full(buf.shape, np.nan, np.float32))
    p = det.probs
    ctx.call("ssdseg_det_loss_scaled", det.y_labels, p.buf, det.y_boxes, det.boxes.buf, p.n, p.h * p.w, p.c, det.w_conf / p.n, det.w_loc / p.n,
             det.conf_loss, det.loc_loss, det.logits.grad, det.boxes.grad, None)
    eng.backward()
    ctx.sync()
    got = [det.logits.grad.download(), det.boxes.grad.download(), det.conf_loss.download(), det.loc_loss.download(), eng.P["grads"].download()]
    for g, w, name in zip(got, want, ("logits.grad", "boxes.grad", "conf_loss", "loc_loss", "bucket")):
        assert np.array_equal(bits(g), bits(w)), name


# ---------------------------------------------------------------------------------------------------------- 9. Keras surface
def test_focal_loss_through_compile_and_fit(ctx, poison, rng):
    """compile(loss={'output-labels': focal_confidence_loss(...)}, metrics={'output-labels': categorical_accuracy(...)}) and two
    one-step fit calls on compact batches with compact validation_data: the history keys are the mined loss's, everything is
    finite, and the first step's `output-labels_loss` is the standalone callable's value on the engine's own targets and
    probabilities"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build(seed=5)
    focal = ssdseglib.losses.focal_confidence_loss(FOCAL_ALPHA, FOCAL_GAMMA)
    compile_det(model, focal, WEIGHTS, metrics={'output-labels': ssdseglib.metrics.categorical_accuracy(classes_weights=(1.0, 1.0, 1.0, 1.0))})

    def compact(n):
        enc, gts, targets = make_targets(rng, boxes, n)
        img = rng.integers(0, 256, (n,) + SHAPE).astype(np.uint8)
        return ssdseglib.datacoder.CompactBatch(img, targets['output-mask'].argmax(-1).astype(np.uint8), gts, np.zeros(n, np.uint8), enc)

    train, val = compact(3), compact(2)
    keys = {'loss', 'output-mask_loss', 'output-labels_loss', 'output-boxes_loss', 'output-labels_categorical_accuracy_metric'}
    for step in range(2):
        hist = model.fit([train], epochs=1, validation_data=[val], verbose=0).history
        assert set(hist) >= keys | {"val_" + k for k in keys}, sorted(hist)
        assert all(len(v) == 1 and np.isfinite(v[0]) for v in hist.values()), hist
        total = sum(WEIGHTS[k] * hist[f"{k}_loss"][0] for k in WEIGHTS)
        assert abs(hist['loss'][0] - total) <= 1e-6 * abs(total)
        if step == 0:
            eng = model._engines[(3, True)]
            det = eng.loss_ops["det"]
            assert det.kind == "focal" and model._engines[(2, "eval")].loss_ops["det"].kind == "focal"
            y, p = det.y_labels.download(), eng.output(1)
            assert y[..., 1:].sum() > 0
            alone = focal(y, p)
            assert alone.shape == (3,) and alone.dtype == np.float32
            assert abs(hist['output-labels_loss'][0] - alone.mean()) <= 1e-5 * abs(alone.mean())
            ref, _ = F.focal_confidence_loss(y, p.astype(np.float32), FOCAL_ALPHA, FOCAL_GAMMA)
            assert rel_err(alone, ref) < 1e-5
