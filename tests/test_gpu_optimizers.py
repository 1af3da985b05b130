"""GPU parity of ssdseg_sgd_step / ssdseg_adamw_step at their edges (through the C-ABI) against their NumPy specifications
(ssdseglib.optimizers._sgd_reference / _adamw_reference, run in float64 on the device's own float32 state), and of the optimizer
surface above them: the engine's dispatch, decay on the right weights, schedules, and resuming a run from a checkpoint.

The bounds are elementwise and derived (sgd_bound, adamw_bound): one relative rounding u = 2^-24 per fp32 operation of the
specification, propagated to first order.  A fused multiply-add only removes a rounding, so contraction stays inside them.
"""
import ctypes as C

import numpy as np
import pytest

from ssdseglib import optimizers as Opt
from tests.test_gpu_full_model import CW, SHAPE, build, make_targets
from tests.test_gpu_training_steps import U, adam_bound, f32
from _guard import guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GRID = 2048 * 256 * 4                  # elements one trip of the optimizer kernels' capped grid covers (csrc/decay_runs.h: decay_blocks)
BIG = GRID + 6                         # one float4 more than that: blocks make a second trip (the last one a partial chunk), and a scalar tail of 2
COUNTS = (1, 3, 4, 5, 1031, BIG)
CAP = 4096                             # SSDSEG_DECAY_RUNS_MAX
LAM = 0.5                              # exact in fp32, and with lr = 0.1 a 5 % change: far above any rounding
LENGTHS = (1, 2, 3, 7, 64, 1000)


# ------------------------------------------------------------------------------------------------------------------ bounds
def sgd_bound(p0, g, v0, lr, mu, nesterov, gscale, lam):
    """fp64 SGD on the kernel's own fp32 inputs -> (p, v, bound on |fp32 p - p|, bound on |fp32 v - v|), elementwise.

    csrc/sgd.hip per element; every fp32 operation rounds once, relative error at most u, errors propagate to first order:
        gk = g gscale                    1 rounding                      |d gk| <= u |gk|
        ll = lr lam                      1 rounding
        d  = ll p                        1 more                          |d d|  <= 2u |d|
        p1 = p - d                       1 more                          |d p1| <= u |p1| + 2u |d|     (lam == 0: p1 = p exactly)
        a  = lr gk                       1 more on top of gk's           |d a|  <= 2u |a|
      momentum == 0:
        p' = p1 - a                                                      |d p'| <= u |p'| + |d p1| + |d a|
      momentum > 0, b = mu v0 (1 rounding, |d b| <= u |b|):
        v' = b - a                                                       |d v'| <= u |v'| + u |b| + 2u |a|
        p' = p1 + v'                                                     |d p'| <= u |p'| + |d p1| + |d v'|
      Nesterov, c = mu v' (|d c| <= u |c| + mu |d v'|), e = c - a (|d e| <= u |e| + |d c| + |d a|):
        p' = p1 + e                                                      |d p'| <= u |p'| + |d p1| + |d e|
    The factor 1.001 covers the O(u^2) terms."""
    p0, g, lam = p0.astype(np.float64), g.astype(np.float64), np.asarray(lam, np.float64)
    gk = g * gscale
    d = (lr * lam) * p0
    p1 = p0 - d
    a = lr * gk
    bp1 = np.where(lam != 0, U * np.abs(p1) + 2 * U * np.abs(d), 0.0)
    ba = 2 * U * np.abs(a)
    if mu == 0:
        p = p1 - a
        return p, None, 1.001 * (U * np.abs(p) + bp1 + ba), None
    b = mu * v0.astype(np.float64)
    v = b - a
    bv = U * np.abs(v) + U * np.abs(b) + ba
    if not nesterov:
        p = p1 + v
        return p, v, 1.001 * (U * np.abs(p) + bp1 + bv), 1.001 * bv
    c = mu * v
    e = c - a
    be = U * np.abs(e) + (U * np.abs(c) + mu * bv) + ba
    p = p1 + e
    return p, v, 1.001 * (U * np.abs(p) + bp1 + be), 1.001 * bv


def adamw_bound(p0, g, m0, v0, t, lr, b1, b2, eps, gscale, lam):
    """adam_bound (tests/test_gpu_training_steps.py) behind the decay p1 = p - (lr lam) p: p1 carries |d p1| <= u |p1| + 2u |d| as
    in sgd_bound (0 where lam == 0), which the final subtraction passes through unchanged.  gscale is a power of two here, so
    g gscale is exact and adam_bound's count of roundings stands."""
    assert np.log2(gscale) == int(np.log2(gscale))
    p0, lam = p0.astype(np.float64), np.asarray(lam, np.float64)
    d = (lr * lam) * p0
    p1 = p0 - d
    p, m, v, bm, bv, bp = adam_bound(p1, g.astype(np.float64) * gscale, m0, v0, t, lr, b1, b2, eps)
    return p, m, v, bm, bv, bp + 1.001 * np.where(lam != 0, U * np.abs(p1) + 2 * U * np.abs(d), 0.0)


# ------------------------------------------------------------------------------------------------------------------ tables
def alternating(rng, count, max_runs):
    """runs of lengths drawn from LENGTHS with lambda alternating LAM, 0, LAM, ... until `count` is covered or max_runs are made"""
    ends, at = [], 0
    while at < count and len(ends) < max_runs:
        at = min(at + int(rng.choice(LENGTHS)), count)
        ends.append(at)
    return np.asarray(ends, np.int64), np.asarray([LAM if i % 2 == 0 else 0.0 for i in range(len(ends))], np.float32)


def table(name, count):
    """(run_end int64, run_decay float32), or None where the count does not allow this table"""
    rng = np.random.default_rng(16)        # (a seed whose first thirteen draws are not the 1000 that would swallow the 1031-element case)
    if name == "none":
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    if name == "one":
        return np.asarray([count], np.int64), np.asarray([LAM], np.float32)
    if name == "small":            # boundaries at 1, 2, 3, 5, 6: every lane of the first float4, and 5 | 6 inside the second
        if count < 2:
            return None
        ends = [e for e in (1, 2, 3, 5, 6) if e < count] + [count]
        return np.asarray(ends, np.int64), np.asarray([LAM if i % 2 == 0 else 0.0 for i in range(len(ends))], np.float32)
    if name == "tail":             # a boundary before the last element: inside the scalar tail where the tail has two or more
        if count < 2:
            return None
        return np.asarray([count - 1, count], np.int64), np.asarray([0.0, LAM], np.float32)
    if name == "alternating":      # (at BIG the cap ends the table short of the count)
        return alternating(rng, count, CAP)
    if name == "cap":              # CAP runs exactly, the last one stretched to the count
        if count < CAP:
            return None
        ends, lams = alternating(rng, count, CAP)
        assert ends.size == CAP
        ends[-1] = count
        return ends, lams
    if name == "short":            # the table ends at half the bucket: the rest takes lambda 0
        if count < 2:
            return None
        return np.asarray([count // 2], np.int64), np.asarray([LAM], np.float32)
    raise KeyError(name)


TABLES = ("none", "one", "small", "tail", "alternating", "cap", "short")
SGD_MODES = {"plain": (0.0, False), "momentum": (0.9, False), "nesterov": (0.9, True)}
EDGE_CASES = [(kind, count, name) for kind in ("momentum", "adamw", "plain", "nesterov") for count in COUNTS for name in TABLES
              if table(name, count) is not None and (kind in ("momentum", "adamw") or name in ("none", "small", "alternating"))]


def test_the_tables_have_the_edges_they_are_named_for():
    ends, lams = table("small", 1031)
    assert ends.tolist() == [1, 2, 3, 5, 6, 1031]
    ends, _ = table("tail", 1031)
    assert ends[0] > 1031 // 4 * 4                              # inside the scalar tail
    ends, _ = table("alternating", 1031)
    assert ends[-1] == 1031 and ends.size > 10 and (ends % 4 != 0).sum() > 5
    ends, lams = table("alternating", BIG)
    assert ends.size == CAP and ends[-1] < BIG                  # short of the count: the remainder takes 0
    ends, lams = table("cap", BIG)
    assert ends.size == CAP and ends[-1] == BIG and (np.diff(ends) > 0).all()
    assert table("short", 1031)[0].tolist() == [515]
    assert BIG // 4 > 2048 * 256 and BIG % 4 == 2               # a second trip and a tail of 2


def upload_table(guards, ends, lams):
    if ends.size == 0:
        return None, None, 0
    return guards.inp(ends), guards.inp(lams), int(ends.size)


def worst(err, bound):
    """(the largest error, the bound of that element)"""
    i = int(np.argmax(err))
    return float(err.ravel()[i]), float(bound.ravel()[i])


def assert_within(name, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    e, b = worst(err, bound)
    over = err > bound
    assert not over.any(), f"{name}: {int(over.sum())} elements beyond their bound, the first {err[over][0]:.3g} against {bound[over][0]:.3g}"
    return f"{name}: err {e:.3g} bound {b:.3g}"


# ------------------------------------------------------------------------------------------------------------------ kernel edges
@pytest.mark.parametrize("kind,count,name", EDGE_CASES)
def test_optimizer_kernel_edges(ctx, guards, kind, count, name):
    """three steps, teacher-forced: before each step the device's own p, v (and m) are downloaded, the specification is run on them
    in float64 with the float32 constants the C-ABI receives, and the step's result is compared elementwise with sgd_bound /
    adamw_bound.  The guards hold that nothing beyond `count` is written, that the table and the gradient are only read."""
    ends, lams = table(name, count)
    rng = np.random.default_rng(count % 1000 + len(name))
    lr, gscale = f32(0.1), 0.5
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-7)
    d_ends, d_lams, nruns = upload_table(guards, ends, lams)
    lam = Opt.expand_runs(ends, lams, count)
    p, g, s1, s2 = (guards.out((count, 1)) for _ in range(4))     # one element per row: the back guard scales with the row pitch
    p.upload(rng.normal(0, 1, count).astype(np.float32))
    s1.upload(rng.normal(0, 0.1, count).astype(np.float32))                  # velocity / m
    s2.upload(rng.uniform(0, 0.01, count).astype(np.float32))                # Adam's v
    n = C.c_size_t(count)
    for step in range(3):
        report = []                                                          # (printed for the last step)
        grad = rng.normal(0, 1, count).astype(np.float32)
        g.upload(grad)
        p0, a0, b0 = p.download().ravel(), s1.download().ravel(), s2.download().ravel()
        if kind == "adamw":
            ctx.call("ssdseg_adamw_step", p, g, s1, s2, n, lr, b1, b2, eps, 5 + step, gscale, d_ends, d_lams, nruns)
            wp, wm, wv, bm, bv, bp = adamw_bound(p0, grad, a0, b0, 5 + step, lr, b1, b2, eps, gscale, lam)
            spec = Opt._adamw_reference(p0.astype(np.float64), grad, a0.astype(np.float64), b0.astype(np.float64), 5 + step, lr, b1, b2, eps,
                                        gscale, ends, lams)
            assert all(np.allclose(a, b, rtol=1e-12, atol=0) for a, b in zip(spec, (wp, wm, wv))), "the bound's fp64 values are not the specification's"
            report += [assert_within("p", p.download().ravel(), spec[0], bp), assert_within("m", s1.download().ravel(), spec[1], bm),
                       assert_within("v", s2.download().ravel(), spec[2], bv)]
        else:
            mu, nesterov = SGD_MODES[kind]
            mu = f32(mu)
            ctx.call("ssdseg_sgd_step", p, g, s1 if mu > 0 else None, n, lr, mu, int(nesterov), gscale, d_ends, d_lams, nruns)
            wp, wv, bp, bv = sgd_bound(p0, grad, a0, lr, mu, nesterov, gscale, lam)
            sp, sv = Opt._sgd_reference(p0.astype(np.float64), grad, a0.astype(np.float64) if mu > 0 else None, lr, mu, nesterov, gscale, ends, lams)
            assert np.allclose(sp, wp, rtol=1e-12, atol=0), "the bound's fp64 values are not the specification's"
            report.append(assert_within("p", p.download().ravel(), sp, bp))
            if mu > 0:
                report.append(assert_within("v", s1.download().ravel(), sv, bv))
            else:
                assert np.array_equal(s1.download().ravel().view(np.uint32), a0.view(np.uint32)), "plain SGD touched the velocity"
        assert np.array_equal(g.download().ravel().view(np.uint32), grad.view(np.uint32)), "the gradient is read only"
        moved = np.abs(p.download().ravel().astype(np.float64) - p0)
        assert moved.max() > 1000 * bp.max(), "the step does not dwarf the rounding"
    print(f"\n{kind} count={count} table={name} ({nruns} runs), third step: " + "; ".join(report))
    ctx.sync()
    guards.check()


# ------------------------------------------------------------------------------------------------------------------ decay placement
@pytest.mark.parametrize("count,name", [(1031, "small"), (1031, "alternating"), (BIG, "cap"), (BIG, "alternating")])
def test_decay_lands_on_exactly_the_right_elements(ctx, guards, count, name):
    """the gradient is zero on a seeded half of the elements, momentum 0, lr 0.1: there the step is the decay alone -- the parameter
    comes back bit for bit where lambda is 0, and 5 % smaller (p - (lr lambda) p within sgd_bound) where lambda is 0.5"""
    ends, lams = table(name, count)
    rng = np.random.default_rng(23)
    lam = Opt.expand_runs(ends, lams, count)
    assert 0.1 < (lam != 0).mean() < 0.9 or name == "small"
    p0 = rng.normal(0, 1, count).astype(np.float32)
    p0[p0 == 0] = 1.0
    grad = rng.normal(0, 1, count).astype(np.float32)
    quiet = rng.uniform(size=count) < 0.5
    grad[quiet] = 0.0
    lr = f32(0.1)
    d_ends, d_lams, nruns = upload_table(guards, ends, lams)
    p = guards.out((count, 1))
    p.upload(p0)
    ctx.call("ssdseg_sgd_step", p, guards.inp(grad.reshape(count, 1)), None, C.c_size_t(count), lr, 0.0, 0, 1.0, d_ends, d_lams, nruns)
    got = p.download().ravel()
    keep, shrink = quiet & (lam == 0), quiet & (lam != 0)
    assert keep.sum() > 0 and shrink.sum() > 0
    assert np.array_equal(got[keep].view(np.uint32), p0[keep].view(np.uint32)), "an element without decay and without gradient changed"
    want, _, bound, _ = sgd_bound(p0, grad, None, lr, 0.0, False, 1.0, lam)
    print("\n" + assert_within(f"decay count={count} table={name}", got, want, bound))
    rel = np.abs(got[shrink].astype(np.float64) - p0[shrink]) / np.abs(p0[shrink])
    assert rel.min() > 0.049 and rel.max() < 0.051, (rel.min(), rel.max())
    ctx.sync()
    guards.check()


# ------------------------------------------------------------------------------------------------------------------ bit identities
@pytest.mark.parametrize("count", [5, 1031])
def test_adamw_without_decay_is_adam_bit_for_bit(ctx, guards, count):
    rng = np.random.default_rng(count)
    zero_ends, _ = alternating(rng, count, CAP)
    zero = (guards.inp(zero_ends), guards.inp(np.zeros(zero_ends.size, np.float32)), int(zero_ends.size))
    state = [rng.normal(0, 1, count).astype(np.float32), rng.normal(0, 0.1, count).astype(np.float32), rng.uniform(0, 0.01, count).astype(np.float32)]
    grads = rng.normal(0, 1, (3, count)).astype(np.float32)
    n, hyper = C.c_size_t(count), (f32(1e-2), f32(0.9), f32(0.999), f32(1e-7))
    results = {}
    for variant in ("adam", "adamw-no-table", "adamw-zero-table"):
        p, m, v, g = (guards.out((count, 1)) for _ in range(4))
        for buf, a in zip((p, m, v), state):
            buf.upload(a)
        for step in range(3):
            g.upload(grads[step])
            if variant == "adam":
                ctx.call("ssdseg_adam_step", p, g, m, v, n, *hyper, 1 + step, 0.125)
            else:
                ctx.call("ssdseg_adamw_step", p, g, m, v, n, *hyper, 1 + step, 0.125, *(zero if variant == "adamw-zero-table" else (None, None, 0)))
        results[variant] = [b.download() for b in (p, m, v)]
    assert not np.array_equal(results["adam"][0].ravel(), state[0])
    for variant in ("adamw-no-table", "adamw-zero-table"):
        for name, a, b in zip("pmv", results["adam"], results[variant]):
            assert np.array_equal(a, b), f"{variant}: {name} differs from ssdseg_adam_step"
    ctx.sync()
    guards.check()


@pytest.mark.parametrize("count", [5, 1031])
@pytest.mark.parametrize("mode", list(SGD_MODES))
def test_sgd_zero_lambda_table_is_no_table(ctx, guards, count, mode):
    rng = np.random.default_rng(count + 1)
    mu, nesterov = SGD_MODES[mode]
    zero_ends, _ = alternating(rng, count, CAP)
    zero = (guards.inp(zero_ends), guards.inp(np.zeros(zero_ends.size, np.float32)), int(zero_ends.size))
    p0, v0 = rng.normal(0, 1, count).astype(np.float32), rng.normal(0, 0.1, count).astype(np.float32)
    grads = rng.normal(0, 1, (3, count)).astype(np.float32)
    results = []
    for tab in ((None, None, 0), zero):
        p, v, g = (guards.out((count, 1)) for _ in range(3))
        p.upload(p0); v.upload(v0)
        for step in range(3):
            g.upload(grads[step])
            ctx.call("ssdseg_sgd_step", p, g, v if mu > 0 else None, C.c_size_t(count), f32(0.05), f32(mu), int(nesterov), 1.0, *tab)
        results.append((p.download(), v.download()))
    assert not np.array_equal(results[0][0].ravel(), p0)
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    ctx.sync()
    guards.check()


# ------------------------------------------------------------------------------------------------------------------ the model
def compile_with(model, optimizer):
    import ssdseglib
    model.compile(optimizer=optimizer,
                  loss={'output-mask': ssdseglib.losses.cross_entropy(classes_weights=CW), 'output-labels': ssdseglib.losses.confidence_loss,
                        'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights={'output-mask': 1.0, 'output-labels': 1.0, 'output-boxes': 1.0})


def batches(rng, boxes, n, batch=3):
    _, _, targets = make_targets(rng, boxes, batch)
    return [(rng.integers(0, 256, (batch,) + SHAPE).astype(np.float32), targets) for _ in range(n)]


def layer_table(model, weight_decay, names):
    """the run table straight from the layers: one run per trainable weight, nothing merged"""
    ends, lams, at = [], [], 0
    for l in model.layers:
        for wname, arr in l.weights.items():
            if wname in l.trainable_names:
                at += arr.size
                ends.append(at)
                lams.append(weight_decay if wname in names else 0.0)
    return np.asarray(ends, np.int64), np.asarray(lams, np.float32)


def test_one_model_step_with_nesterov_sgd_and_weight_decay(ctx, rng):
    """one train_step of the 96x128 model under SGD(momentum 0.9, Nesterov, weight_decay 1e-2): the new parameters and the velocity
    are the float64 specification of the old parameters, the gradient bucket and a zero velocity, within sgd_bound, with the decay
    on `kernel` / `pointwise_kernel` only.  Control: the same with the decay also on BatchNorm's gamma misses the bound."""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    opt = Opt.SGD(momentum=0.9, nesterov=True, weight_decay=1e-2)
    compile_with(model, opt)
    (x, targets), = batches(rng, boxes, 1)
    eng = E.engine_for(model, 3, True)
    p0 = eng.P["params"].download()
    eng.train_step(x, targets, optimizer=opt)
    ctx.sync()
    P, S = eng.P, eng.opt
    assert S.step == 1 and S.lr == 0.01
    g0, got_p, got_v = P["grads"].download(), P["params"].download(), S.slots["velocity"].download()
    assert np.abs(g0).max() > 0
    lr, mu = f32(0.01), f32(0.9)
    ends, lams = layer_table(model, 1e-2, ("kernel", "pointwise_kernel"))
    assert ends[-1] == P["n_tr"] == p0.size and 0 < (lams != 0).sum() < lams.size
    lam = Opt.expand_runs(ends, lams, p0.size)
    sp, sv = Opt._sgd_reference(p0.astype(np.float64), g0, np.zeros(p0.size), lr, mu, True, 1.0, ends, lams)
    wp, wv, bp, bv = sgd_bound(p0, g0, np.zeros_like(p0), lr, mu, True, 1.0, lam)
    assert np.allclose(sp, wp, rtol=1e-12, atol=0)
    print("\nmodel step, Nesterov SGD + decay: " + assert_within("p", got_p, sp, bp) + "; " + assert_within("v", got_v, sv, bv))
    # the engine's cached table is the merged form of the same thing
    (d_ends, d_lams, nruns), = S.decay_tables.values()
    assert nruns < ends.size and np.array_equal(Opt.expand_runs(d_ends.download(), d_lams.download(), p0.size), lam)
    # control
    ends_c, lams_c = layer_table(model, 1e-2, ("kernel", "pointwise_kernel", "gamma"))
    sp_c, _ = Opt._sgd_reference(p0.astype(np.float64), g0, np.zeros(p0.size), lr, mu, True, 1.0, ends_c, lams_c)
    lam_c = Opt.expand_runs(ends_c, lams_c, p0.size)
    _, _, bp_c, _ = sgd_bound(p0, g0, np.zeros_like(p0), lr, mu, True, 1.0, lam_c)
    miss = np.abs(got_p.astype(np.float64) - sp_c) > bp_c
    assert miss.any() and not miss[lam_c == lam].any(), "decay on gamma would have passed too"


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_schedules_reach_the_kernel(ctx, rng, kind):
    """PiecewiseConstantDecay([0, 1], [1e-2, 1e-3, 1e-4]): step k of three runs at values[k] -- within the bound of the specification
    at that rate and beyond it at either neighbour's; fit reports the rate of each epoch's last step as `lr`, and only for a schedule"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    values = [1e-2, 1e-3, 1e-4]
    sched = Opt.PiecewiseConstantDecay([0, 1], values)
    opt = Opt.Adam(learning_rate=sched) if kind == "adam" else Opt.SGD(learning_rate=sched, momentum=0.9)
    compile_with(model, opt)
    data = batches(rng, boxes, 3)
    # fit first: two epochs of one batch are updates 0 and 1
    hist = model.fit(data[:1], epochs=2)
    assert hist.history["lr"] == [f32(1e-2), f32(1e-3)]
    loss_keys = set(hist.history) - {"lr"}
    eng = E.engine_for(model, 3, True)
    P, S = eng.P, eng.opt
    assert S.step == 2
    S.step = 0                                      # the schedule again from its start, on the state the two epochs left
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-7)
    slots = ("m", "v") if kind == "adam" else ("velocity",)
    for k, (x, targets) in enumerate(data):
        ctx.sync()
        p0, s0 = P["params"].download(), [S.slots[s].download() for s in slots]
        eng.train_step(x, targets, optimizer=opt)
        ctx.sync()
        assert S.step == k + 1 and S.lr == values[k]
        g0, got = P["grads"].download(), P["params"].download()

        def at(rate):
            rate = f32(rate)
            if kind == "adam":
                p, _, _, _, _, bp = adam_bound(p0, g0, s0[0], s0[1], k + 1, rate, b1, b2, eps)
            else:
                p, _, bp, _ = sgd_bound(p0, g0, s0[0], rate, f32(0.9), False, 1.0, np.zeros(p0.size))
            return np.abs(got.astype(np.float64) - p), bp

        err, bound = at(values[k])
        e, b = worst(err, bound)
        print(f"\n{kind} update {k} at lr {values[k]:g}: err {e:.3g} bound {b:.3g}")
        assert (err <= bound).all(), f"update {k}: {int((err > bound).sum())} elements beyond the bound at its own rate {values[k]:g}"
        for nb in (k - 1, k + 1):
            if 0 <= nb < 3:
                err, bound = at(values[nb])
                assert (err > bound).any(), f"update {k} also fits the rate of update {nb}"
    # a float rate: the history keys of before, no `lr`
    compile_with(model, Opt.Adam(learning_rate=1e-4) if kind == "adam" else Opt.SGD(learning_rate=1e-3, momentum=0.9))
    hist = model.fit(data[:1], epochs=1)
    assert set(hist.history) == loss_keys and "lr" not in hist.history


def run_snapshot(ctx, eng, slots):
    ctx.sync()
    P = eng.P
    return {"p": P["params"].download(), "s": P["state"].download(), "t": eng.opt.step, **{s: (eng.opt.clip if s == "clip" else eng.opt.slots[s]).download() for s in slots}}


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_resume_from_weights_and_optimizer_state(ctx, rng, kind, tmp_path):
    """four updates in one go == two updates, Model.save + save_state, a freshly built and compiled model, load_weights + load_state,
    two more updates: params, state (the BatchNorm moving statistics), the moments / velocity and the step counter bit for bit.
    Control: load_weights alone (the optimizer state left as it is) gives other parameters."""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)

    def optimizer():
        sched = Opt.PolynomialDecay(1e-2, 4, end_learning_rate=1e-3, power=0.9)
        return Opt.Adam(learning_rate=sched, weight_decay=1e-2) if kind == "adam" else \
            Opt.SGD(learning_rate=sched, momentum=0.9, nesterov=True, weight_decay=1e-2)

    slots = ("m", "v") if kind == "adam" else ("velocity",)

    def fresh():
        boxes, _, model = build()
        compile_with(model, optimizer())
        return boxes, model

    def steps(model, data):
        eng = E.engine_for(model, 3, True)
        for x, targets in data:
            eng.train_step(x, targets, optimizer=model._compiled["optimizer"])
        return eng

    boxes, whole = fresh()
    data = batches(rng, boxes, 4)
    want = run_snapshot(ctx, steps(whole, data), slots)
    assert want["t"] == 4

    _, first = fresh()
    steps(first, data[:2])
    weights, state = str(tmp_path / "weights"), str(tmp_path / "optimizer")
    first.save(weights)
    Opt.save_state(first, state)

    _, second = fresh()
    second.load_weights(weights)
    Opt.load_state(second, state)                    # before its first step: no engine yet
    assert getattr(second, "_engine_params", None) is None
    got = run_snapshot(ctx, steps(second, data[2:]), slots)
    assert got["t"] == 4
    for key in want:
        if key != "t":
            assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), f"{key} differs after the resume"
    assert np.abs(want["p"] - run_snapshot(ctx, E.engine_for(first, 3, True), slots)["p"]).max() > 0      # the last two updates moved something

    # control, on the trained `second`: weights back to the checkpoint, optimizer state and counter left where they are
    second.load_weights(weights)
    ctrl = run_snapshot(ctx, steps(second, data[2:]), slots)
    assert ctrl["t"] == 6 and not np.array_equal(ctrl["p"], want["p"])
