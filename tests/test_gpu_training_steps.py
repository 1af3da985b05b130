"""Training across steps and calls against the fp64 oracle: state that carries over from one step (or one C-ABI call) to the next.

Teacher-forced multi-step parity: before every step the device's own params, state, Adam moments and step counter are downloaded
and loaded into the fp64 oracle, so each step is judged from the state the device is actually in -- the errors of one step do not
build up into the next and every comparison keeps a fixed tolerance.  Per step: the three losses and every parameter gradient
(the bounds of test_full_train_step_parity), the Adam update of the whole bucket (derived bound, see `adam_bound`) and every
BatchNorm's moving statistics (see `moving_bound`).  Sensitivity controls inside the test show that each check could fail: the
oracle gradient at the PREVIOUS step's weights misses the gradient bound by 10x in most layers (a stale transposed or zero-padded
weight copy would be caught), the moving statistics move by more than their bound, and Adam with the step counter t - 1 misses the
Adam bound.  Then the faults of state left behind by one call for the next: deferred column sums after a training step, the 3x3
conv's BatchNorm partial table sized under one dispatch switch and written under another, and back-to-back forward() calls.

Wall time on one MI355X: about 10 s for the whole file (pytest: 8.3 s), most of it the fp64 oracle on 16 CPUs."""

import numpy as np
import pytest

from oracle import np_ops as O
from oracle.np_model import NpModel
from tests.test_gpu_backbone import device_relu_masks, rel
from tests.test_gpu_full_model import CW, SHAPE, build, make_targets
from _guard import poisoned_ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _ctx_poison(poisoned_ctx):
    """every activation, statistics table and workspace region of the engine starts as NaN (tests/_guard.py)"""
    return poisoned_ctx

U = 2.0 ** -24          # unit roundoff of fp32
LR = 1e-2               # large enough that one step moves every gradient well past the 1e-3 bound (sensitivity control)
B1, B2, EPS = 0.9, 0.999, 1e-7
GRAD_TOL = 1e-3


def f32(v):
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------- helpers
def randomise_bn(model, rng):
    for l in model.layers:
        if type(l).__name__ == "BatchNormalization":
            c = l.weights["gamma"].size
            l.weights["gamma"] = rng.uniform(0.7, 1.3, c).astype(np.float32)
            l.weights["beta"] = rng.normal(0, 0.3, c).astype(np.float32)


def compile_model(model):
    import ssdseglib
    model.compile(optimizer=ssdseglib.optimizers.Adam(learning_rate=LR, beta_1=B1, beta_2=B2, epsilon=EPS),
                  loss={'output-mask': ssdseglib.losses.cross_entropy(classes_weights=CW), 'output-labels': ssdseglib.losses.confidence_loss,
                        'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights={'output-mask': 1.0, 'output-labels': 1.0, 'output-boxes': 1.0})


def snapshot(ctx, eng):
    ctx.sync()
    P = eng.P
    return dict(p=P["params"].download(), s=P["state"].download(), m=eng.opt.slots["m"].download(), v=eng.opt.slots["v"].download(), t=eng.opt.step)


def oracle_from_device(model, eng):
    """the fp64 oracle on the weights and moving statistics the device holds now (Keras-shaped slots of the flat buckets)"""
    ref = NpModel(model, dtype=np.float64)
    ref.set_weights_from(lambda l: [eng._bucket_view(l, w).download() for w in l.weights])
    return ref


def oracle_step(ref, x, targets, batch, relu_masks=None):
    p_mask, p_labels, p_boxes = ref.forward(x, training=True)
    l_mask, dmask = O.cross_entropy_loss(targets['output-mask'].astype(np.float64), p_mask, np.asarray(CW, np.float64))
    l_conf, dconf, _ = O.confidence_loss(targets['output-labels'].astype(np.float64), p_labels)
    l_loc, dloc = O.localization_loss(targets['output-boxes'].astype(np.float64), p_boxes)
    grads = ref.backward([dmask / batch, dconf / batch, dloc / batch], relu_masks=relu_masks)
    return dict(mask=l_mask.mean(), conf=l_conf.mean(), loc=l_loc.mean()), grads


NOISE = 1e-6     # fp32 rounding noise allowed (of the model's largest gradient) where the true gradient is zero only in exact arithmetic


def grad_errors(model, eng, ref_grads, ref=None):
    """{layer: max |device - oracle| / largest oracle gradient of the layer}; a layer whose oracle gradient is exactly zero must be
    (numerically) zero on the device too (inf otherwise).  Except at a BatchNorm that normalises ONE value per channel (the image-
    pooling branch of the ASPP at batch 1): its output is beta whatever the input, so its input gradient and the gradient of the
    conv that feeds it are zero in exact arithmetic, and the sum over pixels of the gradient behind a training BatchNorm is zero,
    so its beta gradient is too.  The oracle leaves fp64 rounding there (< 1e-9 of the model's largest gradient), the device fp32
    rounding: those layers are held to NOISE of the model's largest gradient instead (-1.0 in the result)."""
    count1 = set()
    if ref is not None:
        for l in model.layers:
            if type(l).__name__ == "BatchNormalization" and ref.cache[l.name]["count"] == 1:
                count1.add(l.name)
                count1.update(t.layer.name for t in l.inbound)
    top = max(np.abs(g).max() for d in ref_grads.values() for g in d.values())
    errs = {}
    for l in model.layers:
        if not l.weights or not l.trainable_names:
            continue
        got = {w: eng.grad_array(l, w).astype(np.float64) for w in l.trainable_names}
        scale = max(np.abs(ref_grads[l.name][w]).max() for w in l.trainable_names)
        if l.name in count1 and scale <= 1e-9 * top:
            errs[l.name] = -1.0 if all(np.abs(g).max() <= NOISE * top for g in got.values()) else np.inf
            continue
        if scale == 0:
            errs[l.name] = 0.0 if all(np.abs(g).max() < 1e-12 for g in got.values()) else np.inf
            continue
        errs[l.name] = max(np.abs(got[w] - ref_grads[l.name][w]).max() for w in l.trainable_names) / scale
    return errs


def adam_bound(p0, g, m0, v0, t, lr, b1, b2, eps):
    """fp64 Adam on the kernel's own fp32 inputs and constants -> (p, m, v, elementwise bound on |fp32 kernel - fp64|).

    csrc/adam.hip, per element with c1 = 1 - b1, c2 = 1 - b2 (exact in fp32 and fp64 for the fp32 b1, b2 the kernel receives) and
    alpha = lr sqrt(1 - b2^t) / (1 - b1^t) formed in fp64 and rounded once to fp32:
        m = m0 + (g - m0) c1          3 roundings: |dm| <= u (|m| + 2 c1 |g - m0|)
        v = v0 + (g g - v0) c2        4 roundings: |dv| <= u (|v| + c2 (2 |g g - v0| + g g))
        p = p0 - alpha m / (sqrt(v) + eps)
    The step s = alpha m / d, d = sqrt(v) + eps, collects alpha's rounding, the product, sqrtf (counted at 2u: one ulp), the sum
    and the quotient (6u relative), plus the propagated |dm| alpha / d and |dv| / (2 sqrt(v) d) |s|; the subtraction adds
    u |p|.  First order in u (fused multiply-adds only drop roundings); the factor 1.001 covers the O(u^2) terms."""
    c1, c2 = 1.0 - b1, 1.0 - b2
    p, m, v = (a.astype(np.float64) for a in O.adam_step(p0.astype(np.float64), g.astype(np.float64), m0.astype(np.float64),
                                                             v0.astype(np.float64), t, lr=lr, b1=b1, b2=b2, eps=eps))
    g64, m064, v064 = g.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    bm = U * (np.abs(m) + 2 * c1 * np.abs(g64 - m064))
    bv = U * (np.abs(v) + c2 * (2 * np.abs(g64 * g64 - v064) + g64 * g64))
    d = np.sqrt(v) + eps
    s = alpha * m / d
    sv = np.sqrt(v)
    rel_d = np.divide(bv, 2 * sv * d, out=np.zeros_like(bv), where=sv > 0)
    bp = U * np.abs(p) + np.abs(s) * (6 * U + rel_d) + alpha * bm / d
    return p, m, v, 1.001 * bm, 1.001 * bv, 1.001 * bp


BATCH_STAT_TOL = 1e-3   # batch statistics of the fp32 forward vs the fp64 oracle, relative to the channel's RMS (as the outputs)


def moving_bound(mm0, mv0, cache, momentum):
    """O.bn_moving_update(pre-step state, oracle batch statistics) and its bound: the device folds ITS batch statistics, which
    agree with the oracle's to BATCH_STAT_TOL of the channel's RMS r (mean) / 2 r^2 (variance, times the Bessel factor), scaled by
    (1 - momentum); plus fp32 rounding of the update (4u of each term).  r is at least the RMS of the whole layer: the forward's
    errors scale with the tensor, and a channel of ONE value near zero (a 1x1 map at batch 1) has no RMS of its own"""
    mm, mv = O.bn_moving_update(mm0, mv0, cache, momentum=momentum)
    n = cache["count"]
    bessel = n / (n - 1.0) if n > 1 else 1.0
    mean, var = cache["mean"].astype(np.float64), cache["var"].astype(np.float64)
    r2 = var + mean * mean
    r2 = np.maximum(r2, r2.mean())
    k = 1.0 - momentum
    bm = k * BATCH_STAT_TOL * np.sqrt(r2) + 4 * U * (np.abs(mm) + k * np.abs(mean))
    bv = k * bessel * 2 * BATCH_STAT_TOL * r2 + 4 * U * (np.abs(mv) + k * bessel * var)
    return mm, mv, bm, bv


class Checker:
    """one training step on a device engine, judged against the fp64 oracle from the device's pre-step state"""

    def __init__(self, ctx, model):
        self.ctx, self.model = ctx, model
        self.bns = [l for l in model.layers if type(l).__name__ == "BatchNormalization"]
        self.stale_fracs, self.move_fracs, self.adam_fracs = [], [], []
        self.worst = 0.0
        self.prev = None     # (pre-step weights of the previous step, as an oracle) for the stale-weights control

    def step(self, eng, x, targets, stale_control=False):
        ctx, model, batch = self.ctx, self.model, eng.batch
        pre = snapshot(ctx, eng)
        ref = oracle_from_device(model, eng)
        pre_state = {l.name: (ref.weights[l.name]["moving_mean"].copy(), ref.weights[l.name]["moving_variance"].copy()) for l in self.bns}
        eng.set_input(x)
        eng.set_targets(targets)
        eng.forward()
        eng.backward()
        ctx.sync()
        losses, ref_grads = oracle_step(ref, x, targets, batch, relu_masks=device_relu_masks(eng, model))
        got = eng.losses()
        for key, name in (("mask", 'output-mask_loss'), ("conf", 'output-labels_loss'), ("loc", 'output-boxes_loss')):
            assert abs(got[name] - losses[key]) < 1e-3 * abs(losses[key]), (pre["t"] + 1, name, got[name], losses[key])
        errs = grad_errors(model, eng, ref_grads, ref)
        bad = {k: v for k, v in errs.items() if not v < GRAD_TOL}
        assert not bad, f"step {pre['t'] + 1}: gradients off the oracle: {bad}"
        self.worst = max(self.worst, max(errs.values()))
        self.last_errs = errs
        g = eng.P["grads"].download()

        if stale_control:
            # the same step's oracle at the PREVIOUS step's weights: what a stale derived weight copy would compute
            assert self.prev is not None
            _, stale_grads = oracle_step(self.prev, x, targets, batch)
            serr = grad_errors(model, eng, stale_grads)
            live = [k for k in serr if np.isfinite(serr[k]) and serr[k] >= 0 and errs[k] > 0]
            frac = np.mean([serr[k] > 10 * GRAD_TOL for k in live])
            self.stale_fracs.append((frac, float(np.median([serr[k] for k in live]))))
            assert frac > 0.5, f"stale-weights control: only {frac:.0%} of the layers miss the gradient bound by 10x"
        self.prev = ref

        # Adam on the whole bucket, from the device's own p, g, m, v and counter
        opt = model._compiled["optimizer"]
        lr, b1, b2, eps = f32(opt.learning_rate), f32(opt.beta_1), f32(opt.beta_2), f32(opt.epsilon)
        eng.adam_step(lr=opt.learning_rate, beta1=opt.beta_1, beta2=opt.beta_2, eps=opt.epsilon)
        post = snapshot(ctx, eng)
        t = post["t"]
        assert t == pre["t"] + 1
        p, m, v, bm, bv, bp = adam_bound(pre["p"], g, pre["m"], pre["v"], t, lr, b1, b2, eps)
        for name, got_a, want, b in (("adam_m", post["m"], m, bm), ("adam_v", post["v"], v, bv), ("params", post["p"], p, bp)):
            over = np.abs(got_a.astype(np.float64) - want) > b
            assert not over.any(), f"step {t} {name}: {int(over.sum())} elements off the fp64 Adam bound, worst at {int(np.argmax(np.abs(got_a - want) - b))}"
        if t >= 2:      # control: the counter matters -- Adam with t - 1 misses the bound on most updated elements
            p_prev, _, _, _, _, _ = adam_bound(pre["p"], g, pre["m"], pre["v"], t - 1, lr, b1, b2, eps)
            upd = g != 0
            miss = np.abs(post["p"].astype(np.float64) - p_prev)[upd] > bp[upd]
            self.adam_fracs.append(float(miss.mean()))
            assert miss.mean() > 0.9, f"Adam counter control: only {miss.mean():.0%} of the elements tell t from t - 1"

        # moving statistics of every BatchNorm (the zero-padded '1x' ones included: read from the bucket)
        moved = []
        counts = set()
        for l in self.bns:
            c = ref.cache[l.name]
            counts.add(c["count"])
            mm, mv, bmm, bmv = moving_bound(*pre_state[l.name], c, l.momentum)
            got_mm = eng._bucket_view(l, "moving_mean").download().astype(np.float64)
            got_mv = eng._bucket_view(l, "moving_variance").download().astype(np.float64)
            assert (np.abs(got_mm - mm) <= bmm).all(), (t, l.name, "moving_mean", np.abs(got_mm - mm).max(), bmm.max())
            assert (np.abs(got_mv - mv) <= bmv).all(), (t, l.name, "moving_variance", np.abs(got_mv - mv).max(), bmv.max())
            mm0, mv0 = pre_state[l.name]
            moved += list(np.abs(mm - mm0) > bmm) + list(np.abs(mv - mv0) > bmv)
        frac = float(np.mean(moved))
        self.move_fracs.append(frac)
        assert frac > 0.9, f"step {t}: only {frac:.0%} of the moving statistics move by more than their bound"
        return counts


def shufflenet_targets(rng, anchors, batch):
    y_labels = np.zeros((batch, anchors, 4), np.float32)
    y_labels[..., 0] = 1
    y_boxes = np.zeros((batch, anchors, 4), np.float32)
    for b in range(batch):
        pos = rng.choice(anchors, 6, replace=False)
        y_labels[b, pos] = np.eye(4, dtype=np.float32)[rng.integers(1, 4, 6)]
        y_boxes[b, pos] = rng.normal(0, 1, (6, 4)).astype(np.float32)
    y_mask = np.eye(4, dtype=np.float32)[rng.integers(0, 4, (batch,) + SHAPE[:2])]
    return {'output-mask': y_mask, 'output-labels': y_labels, 'output-boxes': y_boxes}


# ------------------------------------------------------------------------------------------------------------ multi-step parity
@pytest.mark.parametrize("case", ["mobilenetv2", "shufflenetv2-1x", "ragged"])
def test_training_steps_teacher_forced(ctx, rng, case):
    """T steps (fresh images and targets each), every step against the fp64 oracle from the device's pre-step state.
    "ragged": two steps on the batch-3 engine, then one on the batch-1 engine `fit` uses for a partial last batch (same counter,
    same moments: Adam at t = 3; its 1x1-map BatchNorms see count 1 and take the unbiased-variance branch's `else`), then an
    inference engine's forward with the device's moving statistics"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    if case == "shufflenetv2-1x":
        from tests.test_gpu_shufflenet import builder
        model = builder(SHAPE, True, True, '1x').get_model_for_training('deeplabv3plus', 'ssdlite', (3, 6, 12))
        for l in model.layers:      # quirk Q1 fixed (bench.py ShuffleNetV2 "q1fixed"): otherwise every gradient is exactly zero
            if type(l).__name__ == "ReLU" and l.max_value == 0.0:
                l.max_value = 6.0
        assert any(pad != c for pad, c in ((E.pad4(l.weights["gamma"].size), l.weights["gamma"].size)
                                           for l in model.layers if type(l).__name__ == "BatchNormalization")), "needs 58-channel BatchNorms"
        boxes = None
    else:
        boxes, _, model = build()
    randomise_bn(model, rng)
    compile_model(model)
    eng = E.engine_for(model, 3, True)
    chk = Checker(ctx, model)

    def targets_for(batch):
        if boxes is None:
            return shufflenet_targets(rng, eng.loss_ops["det"].y_labels.shape[1], batch)
        return make_targets(rng, boxes, batch)[2]

    steps = 2 if case == "ragged" else 4
    for t in range(1, steps + 1):
        x = rng.integers(0, 256, (3,) + SHAPE).astype(np.float32)
        chk.step(eng, x, targets_for(3), stale_control=(t == 2))
    if case == "ragged":
        eng1 = E.engine_for(model, 1, True)
        assert eng1.P is eng.P
        x = rng.integers(0, 256, (1,) + SHAPE).astype(np.float32)
        counts = chk.step(eng1, x, targets_for(1))
        assert -1.0 in chk.last_errs.values(), "the batch-1 step should meet the one-value BatchNorm of the image-pooling branch"
        assert eng.opt.step == 3
        assert 1 in counts and any(c > 1 for c in counts), counts        # both branches of the Bessel correction taken
        # inference forward with the moving statistics the three steps left
        inf = E.Engine(model, 1, training=False, ctx=ctx)
        inf.set_input(x)
        inf.forward()
        ctx.sync()
        ref = oracle_from_device(model, eng)
        r_mask, r_labels, r_boxes = ref.forward(x, training=False)
        assert np.abs(inf.output(0) - r_mask).max() < 1e-3
        assert np.abs(inf.output(1) - r_labels).max() < 1e-3
        assert np.abs(inf.output(2) - r_boxes).max() < 1e-3 * max(1.0, np.abs(r_boxes).max())
    print(f"{case}: worst gradient rel err {chk.worst:.2e}; stale-weights control (share of layers > 1e-2, median err) "
          f"{chk.stale_fracs}; moving statistics moved {chk.move_fracs}; Adam t-1 control {chk.adam_fracs}")


# --------------------------------------------------------------------------------------------- state left behind by one call
def _trained_engine(ctx, rng, seed=31):
    from ssdseglib import _engine as E
    boxes, _, model = build(seed=seed)
    compile_model(model)
    eng = E.Engine(model, 3, training=True, ctx=ctx)
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    x = rng.integers(0, 256, (3,) + SHAPE).astype(np.float32)
    targets = make_targets(rng, boxes, 3)[2]
    return model, eng, x, targets


def test_weight_gradient_entry_points_after_a_training_step(ctx, rng):
    """A training step leaves the context as it found it: after Engine.backward() (deferred column sums), a weight-gradient entry
    point on the same context folds its partial slabs at once, so a consumer that does not join (ssdseg_copy2d) reads the
    finished dW.  Failed before backward() ended deferral: the copy read the destination before the fold (zeros here).  The
    deferral is still on after the step (ssdseg_colsum_defer(1) is how an engine pass starts): the weight-gradient call itself must
    find it off."""
    from ssdseglib import _hip as H
    from tests.test_gpu_conv_ops import make_gview_inputs, make_view_inputs
    model, eng, x, targets = _trained_engine(ctx, rng)
    eng.train_step(x, targets, optimizer=model._compiled["optimizer"])
    ctx.sync()
    # pointwise weight gradient with partial slabs (a PW_CASES shape)
    m, k, n = 153600, 32, 192
    xin, sc, sh, a = make_view_inputs(rng, (m, k), O.ACT_RELU6)
    g, yraw, gs, gt, k1, k0, dy = make_gview_inputs(rng, (m, n), O.ACT_RELU6)
    bufs = [ctx.array(v) for v in (g, yraw, gs, gt, k1, k0)]
    dw, cp = ctx.zeros((k, n)), ctx.zeros((k, n))
    view = H.view(ctx.array(xin), ctx.array(sc), ctx.array(sh), O.ACT_RELU6)
    # (nothing between the two calls: uploads and memsets join the context, which would fold the slabs anyway)
    ctx.call("ssdseg_pwconv_bwd_weight", view, k, H.gview(*bufs, act=O.ACT_RELU6), n, dw, m, k, n)
    ctx.call("ssdseg_copy2d", cp, n, dw, n, k, n)
    want = a.astype(np.float64).T @ dy.astype(np.float64)
    assert rel(cp.download(), want) < 1e-4
    # depthwise backward (dx and dW; slabs of 9 taps x channels)
    nb, h, w, c = 4, 30, 40, 144
    xd, scd, shd, ad = make_view_inputs(rng, (nb, h, w, c), O.ACT_RELU6)
    wd = rng.normal(0, 0.3, (3, 3, c)).astype(np.float32)
    gd = rng.normal(0, 1, (nb, h, w, c)).astype(np.float32)
    ddx, ddw, cpd = ctx.empty((nb, h, w, c)), ctx.zeros((3, 3, c)), ctx.zeros((9, c))
    view, dwd, gvd = H.view(ctx.array(xd), ctx.array(scd), ctx.array(shd), O.ACT_RELU6), ctx.array(wd), H.gview(ctx.array(gd))
    ctx.call("ssdseg_dwconv_bwd", view, dwd, gvd, ddx, ddw, nb, h, w, c, 1, 1, 0)
    ctx.call("ssdseg_copy2d", cpd, c, ddw, c, 9, c)
    _, dw_ref = O.dwconv_bwd(ad.astype(np.float64), wd.astype(np.float64), gd.astype(np.float64), 1, 1)
    assert rel(cpd.download().reshape(3, 3, c), dw_ref) < 1e-4


def test_deferred_column_sum_arena_is_bounded(rng, monkeypatch):
    """With deferral on and no join, a loop of weight-gradient calls folds what is pending once the slab arena reaches its cap
    (SSDSEG_COLSUM_ARENA_MB) instead of allocating 256 MiB chunks without bound; every dW is still right.  (A context of its own:
    the session context's arena may already hold more than the loop needs.)"""
    from ssdseglib import _hip as H
    monkeypatch.setenv("SSDSEG_COLSUM_ARENA_MB", "256")

    def loop(c2):          # (its buffers are gone when it returns, before the context is closed)
        m, k, n = 153600, 32, 192
        xin = rng.normal(0, 1, (m, k)).astype(np.float32)
        gin = rng.normal(0, 1, (m, n)).astype(np.float32)
        dx_, dg = c2.array(xin), c2.array(gin)
        want = xin.astype(np.float64).T @ gin.astype(np.float64)
        outs = [c2.zeros((k, n)) for _ in range(12)]
        c2.colsum_defer(True)
        c2.timing(True)
        c2.timing_reset()
        for i in range(12):                     # 12 x 12 calls with a few MiB of slabs each: more than 256 MiB in all
            for o in outs:
                c2.call("ssdseg_pwconv_bwd_weight", H.view(dx_), k, H.gview(dg), n, o, m, k, n)
        early = c2.timing_report().get("colsum_batch_kernel", {"count": 0})["count"]
        c2.timing(False)
        c2.colsum_defer(False)
        return early, max(rel(o.download(), want) for o in outs)

    c2 = H.Context(0)
    try:
        early, err = loop(c2)
    finally:
        c2.sync()
        c2.close()
    assert err < 1e-4
    assert early >= 1, "the arena cap never folded the pending column sums"


CONV3_FORMS = {"gemm": {"SSDSEG_CONV3_TILE": "0", "SSDSEG_CONV3_NARROW": "0"},
               "tile": {"SSDSEG_CONV3_TILE": "1", "SSDSEG_CONV3_WINOGRAD": "0", "SSDSEG_CONV3_NARROW": "0"},
               "wino": {"SSDSEG_CONV3_TILE": "1", "SSDSEG_CONV3_WINOGRAD": "1", "SSDSEG_CONV3_F4": "0", "SSDSEG_CONV3_NARROW": "0"},
               "wino4": {"SSDSEG_CONV3_TILE": "1", "SSDSEG_CONV3_WINOGRAD": "1", "SSDSEG_CONV3_F4": "1", "SSDSEG_CONV3_NARROW": "0"},
               "narrow": {"SSDSEG_CONV3_NARROW": "1"}}


@pytest.mark.parametrize("n,h,w,cin,cout,sized,launched", [(2, 6, 64, 80, 72, "wino4", "tile"), (2, 6, 64, 80, 72, "tile", "wino4"),
                                                            (2, 6, 64, 80, 72, "gemm", "wino"), (1, 12, 16, 304, 256, "wino4", "gemm"),
                                                            (2, 8, 8, 256, 4, "narrow", "tile"), (18, 120, 22, 256, 4, "tile", "narrow")])
def test_conv3x3_statistics_table_sized_under_another_switch(ctx, rng, monkeypatch, n, h, w, cin, cout, sized, launched):
    """The engine sizes the BatchNorm partial table of a 3x3 conv once; the forward reads the dispatch switches again at every
    launch.  Table sized under one form, forward launched under another: the folded statistics equal the oracle's.  No launch
    happens unless both settings give the same size (test_cpu_cabi_and_host checks that for every setting), so an unfixed build
    fails here without writing past the table.  Failed before the fix: sizes differed (or unwritten rows were folded)."""
    from ssdseglib import _hip as H
    from tests.test_gpu_conv_ops import make_view_inputs

    def parts(form):
        for k in ("SSDSEG_CONV3_TILE", "SSDSEG_CONV3_WINOGRAD", "SSDSEG_CONV3_F4", "SSDSEG_CONV3_NARROW"):
            monkeypatch.delenv(k, raising=False)
        for k, v in CONV3_FORMS[form].items():
            monkeypatch.setenv(k, v)
        return ctx.parts("ssdseg_conv3x3_parts", n, h, w, cin, cout)

    rows_launched = parts(launched)
    rows = parts(sized)
    if rows != rows_launched:
        pytest.fail(f"partial table: {rows} rows sized under '{sized}', {rows_launched} under '{launched}' (no launch made)")
    x, sc, sh, a = make_view_inputs(rng, (n, h, w, cin), O.ACT_RELU6)
    wgt = (rng.normal(0, 1, (3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    stats = ctx.array(np.full((rows, 2, cout), 1e3, np.float32))        # stale rows would show
    y = ctx.empty((n, h, w, cout))
    parts(launched)
    ctx.call("ssdseg_conv3x3_fwd", H.view(ctx.array(x), ctx.array(sc), ctx.array(sh), O.ACT_RELU6), cin, ctx.array(wgt), y, n, h, w, cin, cout, stats)
    y_ref = O.conv2d_fwd(a.astype(np.float64), wgt.astype(np.float64))
    assert rel(y.download(), y_ref) < 5e-5
    st = stats.download().astype(np.float64).sum(axis=0)
    assert np.abs(st[0] - y_ref.sum(axis=(0, 1, 2))).max() < 1e-4 * np.abs(y_ref).sum(axis=(0, 1, 2)).max()
    assert rel(st[1], (y_ref ** 2).sum(axis=(0, 1, 2))) < 1e-4


@pytest.mark.parametrize("side", ["1", "0"])
def test_back_to_back_forward_calls(ctx, rng, monkeypatch, side):
    """forward(); forward(); backward() == forward(); backward() from the same state, bit for bit (gradients, losses), with the
    detection branch on the side stream and with everything on one stream.  The race it guards against (a second forward()
    overwriting trunk activations and weight copies while the first one's detection branch still reads them) is timing-dependent:
    a pass before the fix proved nothing.  The fix, a join at the top of forward(), is correct by construction."""
    monkeypatch.setenv("SSDSEG_DET_SIDE", side)
    model, eng, x, targets = _trained_engine(ctx, rng, seed=37)
    P = eng.P
    eng.train_step(x, targets, optimizer=model._compiled["optimizer"])     # a non-trivial state: moments, moving statistics
    ctx.sync()
    p0, s0 = P["params"].download(), P["state"].download()
    eng.set_input(x)
    eng.set_targets(targets)

    def run(forwards):
        P["params"].upload(p0)
        P["state"].upload(s0)
        for _ in range(forwards):
            eng.forward()
        eng.backward()
        ctx.sync()
        return P["grads"].download(), eng.losses()

    a, b = run(1), run(2)
    assert np.isfinite(a[0]).all() and np.abs(a[0]).max() > 0
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
