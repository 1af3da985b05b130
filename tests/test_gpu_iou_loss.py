"""GPU parity of the IoU-family box regression loss (`ssdseg_loc_loss_iou`, `losses.iou_localization_loss`): the kernels against
the float64 spec of tests/_iou_loss_oracle.py (pinned by test_cpu_iou_loss_oracle.py) fed the same float32 inputs, and the engine
/ Keras surface on top.

Inputs: tests/_iou_loss_cases.py -- every box-carrying anchor of every random case keeps clear of every kink of the loss (asserted
on the CPU), so float32 and float64 take the same branches and no anchor is left out of a comparison: the share excluded is 0.

Error bounds: the spec evaluated in float32 NumPy differs from the spec in float64 on these inputs by at most
    loss      4.4e-7 relative
    d_boxes   4.1e-5 of the case's max |d_boxes|
(worst over every case, kind and smooth_l1_weight; the d_boxes figure comes from the untrained-head sets with the IoU kind and
weight 0, where most gradients are zero and the largest is small; measured and pinned by
test_float32_numpy_error_of_the_spec_on_the_shared_cases, recorded as K.F32_LOSS_REL / K.F32_DBOX_ABS).  The kernel is allowed
4 x these: the margin covers the device's expf, its division and the different reduction order.  Nothing here is derived from
what the kernel gives."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import np_ops as O
from oracle.np_model import NpModel
import _focal_oracle as F
import _iou_loss_cases as K
import _iou_loss_oracle as S
from _guard import guards  # noqa: F401  (fixture)
from tests.test_gpu_backbone import device_relu_masks, rel
from tests.test_gpu_focal_loss import FOCAL_ALPHA, FOCAL_GAMMA, WEIGHTS, bits, c4, poison, randomise_bn  # noqa: F401  (poison: fixture)
from tests.test_gpu_full_model import CW, SHAPE, STDS, build, make_targets

pytestmark = pytest.mark.gpu

LOSS_BOUND = 4 * K.F32_LOSS_REL
DBOX_BOUND = 4 * K.F32_DBOX_ABS
KINDS = [0, 1, 2]


@functools.lru_cache(maxsize=None)
def reference(key, kind, lam):
    """the float64 spec on the float32 inputs of one case, computed once: loss (b,), d loss / d p (b, a, 4)"""
    t, p, an = inputs_of(key)
    loss, d = S.iou_localization_loss(t, p, an, K.STDS, kind, lam)
    loss.setflags(write=False)
    d.setflags(write=False)
    return loss, d


def inputs_of(key):
    if key == "tie":
        return K.tie_case()[:3]
    return K.case(*key)


def run(ctx, guards, ins, shape, kind, lam, loc_scale, present=("loc", "dbox"), stds=K.STDS):
    b, a = shape
    shapes = dict(loc=(b,), dbox=(b, a, 4))
    outs = {k: guards.out(shapes[k]) for k in present}
    ctx.call("ssdseg_loc_loss_iou", *ins, c4(stds), b, a, kind, lam, loc_scale, outs.get("loc"), outs.get("dbox"))
    ctx.sync()
    guards.check()
    for k in present:
        assert guards.unwritten(outs[k]).size == 0, k
    return {k: outs[k].download() for k in present}


def assert_parity(got, loss_ref, d_ref, what, zeros_where_ref=True):
    """prints each figure, then asserts it"""
    assert np.isfinite(got["loc"]).all() and np.isfinite(got["dbox"]).all()
    if not np.abs(loss_ref).max() > 0:
        assert not got["loc"].any() and not got["dbox"].any() and not d_ref.any()
        return
    e_loss = float(np.abs(got["loc"] - loss_ref).max() / np.abs(loss_ref).max())
    e_d = float(np.abs(got["dbox"] - d_ref).max() / np.abs(d_ref).max())
    print(what, f"loss rel {e_loss:.2e} (bound {LOSS_BOUND:.2e})  d_boxes abs / max {e_d:.2e} (bound {DBOX_BOUND:.2e})")
    assert e_loss < LOSS_BOUND
    assert e_d < DBOX_BOUND
    if zeros_where_ref:
        assert not got["dbox"][d_ref == 0].any()


# ------------------------------------------------------------------------------------------------ 1. kernel against the spec
@pytest.mark.parametrize("b,a,pos_frac", K.SHAPES)
@pytest.mark.parametrize("which", K.SETS)
@pytest.mark.parametrize("lam", K.LAMBDAS)
@pytest.mark.parametrize("kind", KINDS)
def test_iou_loss_parity(ctx, guards, kind, lam, which, b, a, pos_frac):
    t, p, an = K.case(b, a, pos_frac, which)
    loc_scale = 0.5 / b
    got = run(ctx, guards, [guards.inp(v) for v in (t, p, an)], (b, a), kind, lam, loc_scale)
    loss_ref, d_ref = reference((b, a, pos_frac, which), kind, lam)
    if pos_frac == 0.0:
        assert not got["loc"].any() and not got["dbox"].any()          # exactly zero: 0 / max(0, 1)
    else:
        assert np.abs(d_ref).max() > 0 or (kind == 0 and lam == 0.0)
    assert not got["dbox"][np.abs(t).sum(-1) == 0].any()               # exact zeros where the anchor carries no box
    assert_parity(got, loss_ref, d_ref * loc_scale, f"kind={kind} lambda={lam} {which} {(b, a, pos_frac)}")


# --------------------------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("lam", K.LAMBDAS)
@pytest.mark.parametrize("kind", KINDS)
def test_iou_loss_ties(ctx, guards, kind, lam):
    """every second box-carrying anchor predicts its target bit for bit: each min / max of those rows is a tie, and the kernel
    sends the derivative where the spec's strict comparison sends it.  The same bounds.  Exact zeros are not asked of the tied
    rows: there the size gradient is I / (U + eps)^2 - 1 / (E + eps) with I = U = E, a cancellation that rounds to an exact zero
    in one precision and not in another; the centre components, which only ties feed, are exactly zero with weight 0."""
    t, p, an, rows = K.tie_case()
    b, a = t.shape[:2]
    loc_scale = 0.5 / b
    got = run(ctx, guards, [guards.inp(v) for v in (t, p, an)], (b, a), kind, lam, loc_scale)
    loss_ref, d_ref = reference("tie", kind, lam)
    assert_parity(got, loss_ref, d_ref * loc_scale, f"ties kind={kind} lambda={lam}", zeros_where_ref=False)
    assert not got["dbox"][np.abs(t).sum(-1) == 0].any()
    if lam == 0.0:
        tied = got["dbox"][rows[:, 0], rows[:, 1]]
        assert not tied[:, :2].any() and not d_ref[rows[:, 0], rows[:, 1], :2].any()


# -------------------------------------------------------------------------------------------------------------- 3. clamps
@pytest.mark.parametrize("kind", KINDS)
def test_iou_loss_clamped_sizes_have_exactly_zero_gradient(ctx, guards, kind):
    """an untrained head, smooth_l1_weight 0: wherever the raw predicted size is <= 0 its gradient component is exactly 0"""
    t, p, an = K.clamp_case()
    b, a = t.shape[:2]
    got = run(ctx, guards, [guards.inp(v) for v in (t, p, an)], (b, a), kind, 0.0, 0.5 / b)
    q = S.decode(p.astype(np.float64), an.astype(np.float64), K.STDS)
    box = np.abs(t).sum(-1) > 0
    assert ((q["rw"] <= 0) & box).sum() > 10 and ((q["rh"] <= 0) & box).sum() > 10
    assert not got["dbox"][..., 2][q["rw"] <= 0].any()
    assert not got["dbox"][..., 3][q["rh"] <= 0].any()
    assert got["dbox"][..., 2][(q["rw"] > 0) & (q["rh"] > 0) & box].any()


# ---------------------------------------------------------------------------------------------------- 4. optional outputs
def test_iou_loss_optional_outputs(ctx, guards):
    """loss only (validation, the standalone callable) and gradient only: what is present is bit-identical to the full call,
    everything present is written, no guard is touched"""
    b, a, pos_frac = 2, 9600, 0.01
    ins = [guards.inp(v) for v in K.case(b, a, pos_frac, "near")]
    full = run(ctx, guards, ins, (b, a), 1, 1.0, 0.5 / b)
    assert np.abs(full["dbox"]).max() > 0 and np.abs(full["loc"]).min() > 0
    for present in (("loc",), ("dbox",)):
        part = run(ctx, guards, ins, (b, a), 1, 1.0, 0.5 / b, present)
        for k in present:
            assert np.array_equal(bits(part[k]), bits(full[k])), (present, k)


def test_iou_loss_rejects_bad_arguments(ctx, guards):
    """an argument error of the call, before any launch: the outputs still show as unwritten"""
    from ssdseglib import _hip as H
    b, a = 1, 37
    ins = [guards.inp(v) for v in K.case(b, a, 0.1, "near")]
    loc, dbox = guards.out(b), guards.out((b, a, 4))
    nan, inf = float("nan"), float("inf")
    good = dict(stds=K.STDS, a=a, kind=1, lam=1.0, loc_scale=1.0)
    for bad in (dict(kind=3), dict(kind=-1), dict(lam=-1.0), dict(lam=nan), dict(stds=(0.1, 0.0, 0.2, 0.2)), dict(stds=(0.1, 0.1, inf, 0.2)),
                dict(stds=(nan, 0.1, 0.2, 0.2)), dict(a=0), dict(loc_scale=inf)):
        kw = dict(good, **bad)
        with pytest.raises(H.SsdsegError):
            ctx.call("ssdseg_loc_loss_iou", *ins, c4(kw["stds"]), b, kw["a"], kw["kind"], kw["lam"], kw["loc_scale"], loc, dbox)
    with pytest.raises(H.SsdsegError):
        ctx.call("ssdseg_loc_loss_iou", ins[0], ins[1], None, c4(K.STDS), b, a, 1, 1.0, 1.0, loc, dbox)
    ctx.sync()
    assert guards.unwritten(loc).shape[0] == b and guards.unwritten(dbox).shape[0] == b * a * 4


# --------------------------------------------------------------------------------------------------------- 5. determinism
def test_iou_loss_is_deterministic(ctx, guards):
    b, a, pos_frac = 2, 9600, 0.01
    ins = [guards.inp(v) for v in K.case(b, a, pos_frac, "near")]
    first = run(ctx, guards, ins, (b, a), 2, 1.0, 0.5 / b)
    second = run(ctx, guards, ins, (b, a), 2, 1.0, 0.5 / b)
    for k in ("loc", "dbox"):
        assert np.array_equal(bits(first[k]), bits(second[k])), k


# ------------------------------------------------------------------------------------------------------ engine-level tests
def model_boxes(boxes):
    return [boxes.get_boxes_coordinates_center_x('ssd'), boxes.get_boxes_coordinates_center_y('ssd'),
            boxes.get_boxes_coordinates_width('ssd'), boxes.get_boxes_coordinates_height('ssd')]


def compile_iou(model, conf_loss, loc_loss, weights, metrics=None):
    import ssdseglib
    model.compile(optimizer=ssdseglib.optimizers.Adam(learning_rate=1e-4),
                  loss={'output-mask': ssdseglib.losses.cross_entropy(classes_weights=CW), 'output-labels': conf_loss, 'output-boxes': loc_loss},
                  loss_weights=weights, metrics=metrics)


class Spy:
    """the (name, args) of every ctx.call made inside `with spying(...)`"""

    def __init__(self):
        self.calls = []

    def named(self, name):
        return [args for n, args in self.calls if n == name]


@contextlib.contextmanager
def spying(ctx, monkeypatch):
    spy, real = Spy(), ctx.call

    def call(name, *args):
        spy.calls.append((name, args))
        return real(name, *args)

    with monkeypatch.context() as m:
        m.setattr(ctx, "call", call)
        yield spy


# -------------------------------------------------------------------------------------------------- 6. whole-step parity
@pytest.mark.parametrize("conf_kind", ["focal", "mined"])
def test_full_train_step_parity_with_the_giou_loss(ctx, poison, rng, monkeypatch, conf_kind):
    """test_full_train_step_parity_with_unequal_detection_weights' set-up and bounds (loss_weights 1 / 2 / 0.5) with
    iou_localization_loss(giou, smooth_l1_weight 1) on 'output-boxes' and the focal (or the mined) confidence loss: outputs, the
    three losses, the weighted total and every parameter gradient against the fp64 oracle with the spec's d loc.  The calls of the
    forward pass: the confidence entry gets NULL for both localization outputs, `ssdseg_loc_loss_iou` runs once."""
    import ssdseglib
    from ssdseglib import _engine as E
    batch = 3
    boxes, builder, model = build()
    randomise_bn(model, rng)
    enc, gts, targets = make_targets(rng, boxes, batch)
    assert targets['output-labels'][..., 1:].sum() > 0, "test needs at least one positive anchor"
    conf_loss = ssdseglib.losses.focal_confidence_loss(FOCAL_ALPHA, FOCAL_GAMMA) if conf_kind == "focal" else ssdseglib.losses.confidence_loss
    giou = ssdseglib.losses.iou_localization_loss(*model_boxes(boxes), STDS, kind="giou", smooth_l1_weight=1.0)
    compile_iou(model, conf_loss, giou, WEIGHTS)
    E.Engine.keep_mask_probabilities = True         # (so that output(0) can be compared)
    try:
        eng = E.Engine(model, batch, training=True, ctx=ctx)
    finally:
        E.Engine.keep_mask_probabilities = False
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    det = eng.loss_ops["det"]
    assert det.loc is giou and det.loc_kind == 1 and [r.kind for r in eng._loss_names] == ["mask", "conf", "loc"]
    x = rng.integers(0, 256, (batch,) + SHAPE).astype(np.float32)

    ref = NpModel(model, dtype=np.float64)
    p_mask, p_labels, p_boxes = ref.forward(x, training=True)
    l_mask, dmask = O.cross_entropy_loss(targets['output-mask'].astype(np.float64), p_mask, np.asarray(CW, np.float64))
    y_labels = targets['output-labels'].astype(np.float64)
    if conf_kind == "focal":
        l_conf, dconf = F.focal_confidence_loss(y_labels, p_labels, FOCAL_ALPHA, FOCAL_GAMMA)
    else:
        l_conf, dconf, _ = O.confidence_loss(y_labels, p_labels)
    anchors = np.stack([np.asarray(v, np.float32).reshape(-1) for v in model_boxes(boxes)], axis=1)
    y_boxes = targets['output-boxes'].astype(np.float64)
    assert (np.abs(y_boxes).sum(-1) > 0).sum() > 0
    l_loc, dloc = S.iou_localization_loss(y_boxes, p_boxes, anchors, STDS, "giou", 1.0)
    w_mask, w_conf, w_loc = (WEIGHTS[k] for k in ('output-mask', 'output-labels', 'output-boxes'))

    eng.set_input(x)
    eng.set_targets(targets)
    with spying(ctx, monkeypatch) as spy:
        eng.forward()
    iou_calls = spy.named("ssdseg_loc_loss_iou")
    assert len(iou_calls) == 1 and iou_calls[0][9] is det.loc_loss and iou_calls[0][10] is not None      # (loc_loss, d_boxes)
    assert iou_calls[0][6] == 1 and iou_calls[0][7] == 1.0 and iou_calls[0][8] == w_loc / batch             # kind, weight, loc_scale
    if conf_kind == "focal":
        (args,) = spy.named("ssdseg_det_loss_focal")
        assert args[11] is det.conf_loss and args[12] is None and args[13] is not None and args[14] is None
        assert not spy.named("ssdseg_det_loss") and not spy.named("ssdseg_det_loss_scaled")
    else:
        (args,) = spy.named("ssdseg_det_loss")
        assert args[7] == w_conf / batch and args[8] is det.conf_loss and args[9] is None and args[10] is not None and args[11] is None
        assert not spy.named("ssdseg_det_loss_focal") and not spy.named("ssdseg_det_loss_scaled")
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


# ---------------------------------------------------------------------------------------------- 7. what the engine accepts
def test_engine_binds_the_iou_loss_to_the_boxes_output_only(ctx, poison, rng, monkeypatch):
    """ValueError on 'output-labels' and for a default-box count that is not the head's; and with `localization_loss` compiled
    the step never calls `ssdseg_loc_loss_iou`: the fused entry keeps both localization outputs"""
    import ssdseglib
    from ssdseglib import _engine as E
    batch = 3
    boxes, builder, model = build(seed=23)
    enc, gts, targets = make_targets(rng, boxes, batch)
    giou = ssdseglib.losses.iou_localization_loss(*model_boxes(boxes), STDS)
    eng = E.Engine(model, batch, training=True, ctx=ctx)
    ce = ssdseglib.losses.cross_entropy(classes_weights=CW)
    with pytest.raises(ValueError):
        eng.configure_losses({'output-mask': ce, 'output-labels': giou, 'output-boxes': ssdseglib.losses.localization_loss}, {})
    short = ssdseglib.losses.iou_localization_loss(*[v[:-6] for v in model_boxes(boxes)], STDS)
    with pytest.raises(ValueError):
        eng.configure_losses({'output-mask': ce, 'output-labels': ssdseglib.losses.confidence_loss, 'output-boxes': short}, {})
    compile_iou(model, ssdseglib.losses.confidence_loss, ssdseglib.losses.localization_loss, WEIGHTS)
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    det = eng.loss_ops["det"]
    assert det.loc is None
    eng.set_input(rng.integers(0, 256, (batch,) + SHAPE).astype(np.float32))
    eng.set_targets(targets)
    with spying(ctx, monkeypatch) as spy:
        eng.forward()
    assert not spy.named("ssdseg_loc_loss_iou")
    (args,) = spy.named("ssdseg_det_loss_scaled")
    assert args[10] is det.loc_loss and args[12] is not None                # (loc_loss, d_boxes of the fused entry)
    assert np.isfinite(eng.losses()['output-boxes_loss'])


# ---------------------------------------------------------------------------------------------------------- 8. Keras surface
def test_iou_loss_through_compile_and_fit(ctx, poison, rng):
    """compile(loss={'output-boxes': iou_localization_loss(...)}, metrics={'output-boxes': jaccard_iou_bounding_boxes(...)}) and two
    one-step fit calls on compact batches with compact validation_data: the history keys are localization_loss's, everything is
    finite, the first step's `output-boxes_loss` is the standalone callable's value on the engine's own targets and offsets, and the
    evaluation engine's op carries the same loss"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build(seed=5)
    giou = ssdseglib.losses.iou_localization_loss(*model_boxes(boxes), STDS, kind="giou", smooth_l1_weight=1.0)
    focal = ssdseglib.losses.focal_confidence_loss(FOCAL_ALPHA, FOCAL_GAMMA)
    compile_iou(model, focal, giou, WEIGHTS, metrics={'output-boxes': ssdseglib.metrics.jaccard_iou_bounding_boxes(*model_boxes(boxes), STDS)})

    def compact(n):
        for _ in range(20):     # the box metric is NaN for an image without a matched anchor (quirk Q10): every image gets one
            enc, gts, targets = make_targets(rng, boxes, n)
            if (np.abs(targets['output-boxes']).sum(-1) > 0).any(-1).all():
                break
        else:
            raise AssertionError("no target set with a matched anchor in every image")
        img = rng.integers(0, 256, (n,) + SHAPE).astype(np.uint8)
        return ssdseglib.datacoder.CompactBatch(img, targets['output-mask'].argmax(-1).astype(np.uint8), gts, np.zeros(n, np.uint8), enc)

    train, val = compact(3), compact(2)
    keys = {'loss', 'output-mask_loss', 'output-labels_loss', 'output-boxes_loss', 'output-boxes_jaccard_iou_bounding_boxes_metric'}
    for step in range(2):
        hist = model.fit([train], epochs=1, validation_data=[val], verbose=0).history
        assert set(hist) == keys | {"val_" + k for k in keys}, sorted(hist)
        assert all(len(v) == 1 and np.isfinite(v[0]) for v in hist.values()), hist
        total = sum(WEIGHTS[k] * hist[f"{k}_loss"][0] for k in WEIGHTS)
        assert abs(hist['loss'][0] - total) <= 1e-6 * abs(total)
        if step == 0:
            eng = model._engines[(3, True)]
            det = eng.loss_ops["det"]
            ev = model._engines[(2, "eval")].loss_ops["det"]
            assert det.loc is giou and det.loc_kind == 1 and ev.loc is giou and ev.loc_kind == 1 and ev.kind == det.kind == "focal"
            y, p = det.y_boxes.download(), eng.output(2)
            assert (np.abs(y).sum(-1) > 0).sum() > 0
            alone = giou(y, p)
            assert alone.shape == (3,) and alone.dtype == np.float32
            assert abs(hist['output-boxes_loss'][0] - alone.mean()) <= 1e-5 * abs(alone.mean())
            anchors = np.stack([np.asarray(v, np.float32).reshape(-1) for v in model_boxes(boxes)], axis=1)
            ref, _ = S.iou_localization_loss(y, p.astype(np.float32), anchors, STDS, "giou", 1.0)
            assert np.abs(alone - ref).max() < 1e-5 * np.abs(ref).max()
