"""GPU parity of gradient clipping and the EMA of the weights: ssdseg_grad_norm, ssdseg_sgd_step_clipped / ssdseg_adamw_step_clipped
and ssdseg_ema_update at their edges through the C-ABI, against their NumPy specifications in float64 on the device's own float32
state (ssdseglib.optimizers._clip_reference / _sgd_reference / _adamw_reference / _ema_reference), and the surface above them:
the engine's dispatch, fit's `grad_norm`, averaged_weights, and resuming a run with clipping and EMA from a checkpoint.

Bounds are derived as in tests/test_gpu_optimizers.py: one relative rounding u = 2^-24 per fp32 operation of the specification, to
first order, times 1.001.  The clip enters them as follows.  g' = clampv((g gscale) s, c): with gscale a power of two the first
product is exact, the product with s rounds once -- the one rounding sgd_bound grants `gk = g gscale` -- and the clamp rounds
nothing (c is an fp32 number, and |clampv(x~) - clampv(x)| <= |x~ - x|).  So the bounds are sgd_bound / adamw_bound called with the
float64 g' as the gradient and gscale = 1.  For AdamW s = 0.25 makes g' exact, as adam_bound assumes of its gradient.
"""
import ctypes as C
import math

import numpy as np
import pytest

from ssdseglib import optimizers as Opt
from tests.test_gpu_full_model import build
from tests.test_gpu_optimizers import (BIG, SGD_MODES, adamw_bound, assert_within, batches, compile_with, layer_table, run_snapshot, sgd_bound,
                                       table, upload_table)
from tests.test_gpu_training_steps import U, f32
from _guard import BODY_WORD, guards  # noqa: F401  (guards: fixture)

pytestmark = pytest.mark.gpu

INF = math.inf
NORM_COUNTS = (0, 1, 3, 4, 5, 1031, BIG)      # BIG: a second trip of the capped grid, a partial last chunk, a scalar tail of 2


def ulps(a, b):
    """distance in fp32 ulps of two finite floats of the same sign"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def clamp64(x, c):
    return np.where(x < -c, -c, np.where(x > c, c, x))


# ------------------------------------------------------------------------------------------------------------------ (a) the norm
def norm_bucket(data, count):
    rng = np.random.default_rng(count % 1000 + 7)
    if data == "normal":
        return rng.normal(0, 1, count).astype(np.float32)
    if data == "zeros":
        return np.zeros(count, np.float32)
    g = np.full(count, 1e-30, np.float32)          # squares underflow fp32 (1e-60) ...
    if count:
        g[count // 2] = 1e30                       # ... and this one's overflows it (1e60); neither does in double
    return g


@pytest.mark.parametrize("data", ["normal", "adversarial", "zeros"])
@pytest.mark.parametrize("count", NORM_COUNTS)
def test_grad_norm_edges(ctx, guards, count, data):
    """out[0] within 1 fp32 ulp of the float64 norm rounded to float (the double sum's error, n 2^-53 <= 2^-32 relative here, can only
    move the final rounding); out[1] within 1 ulp of the float64 factor at half the norm, exactly 1 where nothing clips; grad_scale
    0.5 halves the norm exactly; two calls give the same 8 bytes; every partial is written, nothing else is."""
    g = norm_bucket(data, count)
    nparts = ctx.lib.ssdseg_grad_norm_parts(count)
    assert 1 <= nparts <= 2048
    d_g = guards.inp(g.reshape(count, 1) if count else np.zeros((1, 1), np.float32))
    partials, out = guards.out((nparts,), np.float64), guards.out((2,))
    n = C.c_size_t(count)

    def run(gscale, clip_norm):
        guards.repoison(out)
        guards.repoison(partials)
        ctx.call("ssdseg_grad_norm", d_g, n, gscale, clip_norm, partials, out)
        got = out.download()
        if count:
            assert np.isfinite(partials.download()).all(), "a partial was not written"
        else:
            assert (bits(partials.download()) == BODY_WORD).all(), "an empty bucket wrote a partial"
        return got

    norm64, _ = Opt._clip_reference(g, 1.0, None)
    assert norm64 == pytest.approx(math.sqrt(float(np.sum(g.astype(np.float64) ** 2))), rel=1e-12)     # (another order of the same float64 sum)
    first = run(1.0, f32(norm64 / 2))
    if norm64 == 0:
        assert bits(first).tolist() == bits(np.asarray([0.0, 1.0], np.float32)).tolist(), "zero bucket: norm 0, factor exactly 1 (no 0/0)"
    else:
        assert ulps(first[0], norm64) <= 1, (first[0], norm64)
        _, factor64 = Opt._clip_reference(g, 1.0, f32(norm64 / 2))
        assert 0.49 < factor64 < 0.51 and ulps(first[1], factor64) <= 1, (first[1], factor64)
    print(f"\ngrad_norm count={count} {data}: norm {first[0]!r} (float64 {norm64!r}), factor {first[1]!r}, {nparts} partials")
    again = run(1.0, f32(norm64 / 2))
    assert bits(again).tolist() == bits(first).tolist(), "two calls on the same bucket differ"
    for off in (f32(norm64 * 2), 0.0, -1.0, INF, math.nan):
        got = run(1.0, off)
        assert bits(got[1:]).tolist() == bits(np.ones(1, np.float32)).tolist(), f"clip_norm {off}: the factor is not exactly 1"
        assert bits(got[:1]).tolist() == bits(first[:1]).tolist()
    for gscale in (0.5, -0.5):
        got = run(gscale, 0.0)
        assert got[0] == np.float32(0.5) * first[0], "grad_scale 0.5 does not halve the norm exactly"
    ctx.sync()
    guards.check()


# ------------------------------------------------------------------------------------------------------------------ (b) clipped steps
CLIP_COUNTS = (5, 1031, BIG)
CLIP_CASES = [(kind, count, name) for kind in ("plain", "momentum", "nesterov", "adamw") for count in CLIP_COUNTS
              for name in ("none", "small", "alternating")]
# g ~ N(0, 1), g' = g gscale s; P(|z| > 0.967) = 1/3
S_SGD, S_ADAM, GSCALE = f32(0.37), 0.25, 0.5
C_SGD, C_ADAM = f32(0.967 * GSCALE * S_SGD), f32(0.967 * GSCALE * S_ADAM)


@pytest.mark.parametrize("kind,count,name", CLIP_CASES)
def test_clipped_step_edges(ctx, guards, kind, count, name):
    """three teacher-forced steps of the *_clipped entries against the float64 specification on the device's own state, the factor
    uploaded by the test (s = 0.37 for SGD: one rounding; 0.25 for AdamW: exact), about a third of |g'| clamped.  Control: the
    specification without the clip misses the bound.  The factor buffer, the table and the gradient are only read."""
    ends, lams = table(name, count)
    rng = np.random.default_rng(count % 1000 + len(name) + 3)
    lr = f32(0.1)
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-7)
    s, c = (S_ADAM, C_ADAM) if kind == "adamw" else (S_SGD, C_SGD)
    d_s = guards.inp(np.asarray([s], np.float32))
    d_ends, d_lams, nruns = upload_table(guards, ends, lams)
    lam = Opt.expand_runs(ends, lams, count)
    p, g, s1, s2 = (guards.out((count, 1)) for _ in range(4))
    p.upload(rng.normal(0, 1, count).astype(np.float32))
    s1.upload(rng.normal(0, 0.1, count).astype(np.float32))                  # velocity / m
    s2.upload(rng.uniform(0, 0.01, count).astype(np.float32))                # Adam's v
    n = C.c_size_t(count)
    for step in range(3):
        report = []
        grad = rng.normal(0, 1, count).astype(np.float32)
        g.upload(grad)
        p0, a0, b0 = p.download().ravel(), s1.download().ravel(), s2.download().ravel()
        geff = clamp64(grad.astype(np.float64) * GSCALE * s, c)              # the float64 g'
        clamped = float((np.abs(geff) == c).mean())
        assert count < 1000 or 0.28 < clamped < 0.39, clamped
        if kind == "adamw":
            ctx.call("ssdseg_adamw_step_clipped", p, g, s1, s2, n, lr, b1, b2, eps, 5 + step, GSCALE, d_ends, d_lams, nruns, d_s, c)
            wp, wm, wv, bm, bv, bp = adamw_bound(p0, geff, a0, b0, 5 + step, lr, b1, b2, eps, 1.0, lam)
            args = (p0.astype(np.float64), grad, a0.astype(np.float64), b0.astype(np.float64), 5 + step, lr, b1, b2, eps, GSCALE, ends, lams)
            spec = Opt._adamw_reference(*args, clip_scale=s, clip_value=c)
            assert all(np.allclose(a, b, rtol=1e-12, atol=0) for a, b in zip(spec, (wp, wm, wv))), "the bound's fp64 values are not the specification's"
            got_p, got_m = p.download().ravel(), s1.download().ravel()
            report += [assert_within("p", got_p, spec[0], bp), assert_within("m", got_m, spec[1], bm),
                       assert_within("v", s2.download().ravel(), spec[2], bv)]
            plain = Opt._adamw_reference(*args)
            assert (np.abs(got_m - plain[1]) > bm).any(), "the unclipped specification passes too"
        else:
            mu, nesterov = SGD_MODES[kind]
            mu = f32(mu)
            ctx.call("ssdseg_sgd_step_clipped", p, g, s1 if mu > 0 else None, n, lr, mu, int(nesterov), GSCALE, d_ends, d_lams, nruns, d_s, c)
            wp, wv, bp, bv = sgd_bound(p0, geff, a0, lr, mu, nesterov, 1.0, lam)
            args = (p0.astype(np.float64), grad, a0.astype(np.float64) if mu > 0 else None, lr, mu, nesterov, GSCALE, ends, lams)
            sp, sv = Opt._sgd_reference(*args, clip_scale=s, clip_value=c)
            assert np.allclose(sp, wp, rtol=1e-12, atol=0), "the bound's fp64 values are not the specification's"
            got_p = p.download().ravel()
            report.append(assert_within("p", got_p, sp, bp))
            if mu > 0:
                report.append(assert_within("v", s1.download().ravel(), sv, bv))
            else:
                assert np.array_equal(bits(s1.download().ravel()), bits(a0)), "plain SGD touched the velocity"
            plain, _ = Opt._sgd_reference(*args)
            assert (np.abs(got_p - plain) > bp).any(), "the unclipped specification passes too"
        assert np.array_equal(bits(g.download().ravel()), bits(grad)), "the gradient is read only"
    print(f"\nclipped {kind} count={count} table={name} ({nruns} runs), third step, {100 * clamped:.0f} % clamped: " + "; ".join(report))
    ctx.sync()
    guards.check()


def test_clampv_passes_nan_and_infinities(ctx, guards):
    """tf.clip_by_value semantics: NaN in, NaN out (fminf(fmaxf(..)) would give c); +-inf clamp to +-c; c = +inf is the identity"""
    grad = np.asarray([math.nan, INF, -INF, 3.0, -3.0, 0.25, -0.0], np.float32)
    want = np.asarray([math.nan, 1.0, -1.0, 1.0, -1.0, 0.25, -0.0], np.float32)
    p = guards.out((grad.size, 1))
    p.upload(np.zeros(grad.size, np.float32))
    ctx.call("ssdseg_sgd_step_clipped", p, guards.inp(grad.reshape(-1, 1)), None, C.c_size_t(grad.size), 1.0, 0.0, 0, 1.0, None, None, 0, None, 1.0)
    got = -p.download().ravel()                     # lr 1, momentum 0: p = 0 - g'
    assert np.isnan(got[0]) and np.array_equal(got[1:], want[1:]), got


# ------------------------------------------------------------------------------------------------------------------ (c) identity
@pytest.mark.parametrize("count", [5, 1031])
@pytest.mark.parametrize("kind", ["plain", "momentum", "nesterov", "adamw"])
def test_factor_one_and_no_clamp_is_the_unclipped_entry_bit_for_bit(ctx, guards, kind, count):
    """*clip_scale == 1.0f (and a NULL factor) with clip_value == +inf: three steps equal ssdseg_sgd_step / ssdseg_adamw_step bit for
    bit -- a step that does not clip does not perturb a run.  SGD at grad_scale 1/3: its g' only ever enters products.  AdamW at
    grad_scale 0.125, as the AdamW-is-Adam identity of tests/test_gpu_optimizers.py: the unclipped kernel's m update contracts
    g * grad_scale into a fused multiply-add, so the identity needs that product to be exact (a power-of-two grad_scale)."""
    rng = np.random.default_rng(count + 5)
    ends, lams = table("alternating", count)
    tab = upload_table(guards, ends, lams)
    one = guards.inp(np.ones(1, np.float32))
    state = [rng.normal(0, 1, count).astype(np.float32), rng.normal(0, 0.1, count).astype(np.float32), rng.uniform(0, 0.01, count).astype(np.float32)]
    grads = rng.normal(0, 1, (3, count)).astype(np.float32)
    n = C.c_size_t(count)
    results = {}
    for variant in ("unclipped", "factor-one", "null-factor"):
        p, a, b, g = (guards.out((count, 1)) for _ in range(4))
        for buf, arr in zip((p, a, b), state):
            buf.upload(arr)
        clip = () if variant == "unclipped" else (one if variant == "factor-one" else None, INF)
        for step in range(3):
            g.upload(grads[step])
            if kind == "adamw":
                ctx.call("ssdseg_adamw_step" + ("_clipped" if clip else ""), p, g, a, b, n, f32(1e-2), f32(0.9), f32(0.999), f32(1e-7), 1 + step,
                         0.125, *tab, *clip)
            else:
                mu, nesterov = SGD_MODES[kind]
                ctx.call("ssdseg_sgd_step" + ("_clipped" if clip else ""), p, g, a if mu > 0 else None, n, f32(0.05), f32(mu), int(nesterov),
                         f32(1.0 / 3.0), *tab, *clip)
        results[variant] = [x.download() for x in (p, a, b)]
    assert not np.array_equal(results["unclipped"][0].ravel(), state[0])
    for variant in ("factor-one", "null-factor"):
        for name, x, y in zip(("p", "velocity / m", "v"), results["unclipped"], results[variant]):
            assert np.array_equal(bits(x), bits(y)), f"{variant}: {name} differs from the unclipped entry"
    ctx.sync()
    guards.check()


# ------------------------------------------------------------------------------------------------------------------ (d) EMA
def ema_bound(e0, p, momentum):
    """float64 ema' = e + (p - e) w, w = fl32(1 - momentum) as the entry forms it, and the bound of three roundings:
        d = p - e        |dd| <= u |d|
        t = d w          |dt| <= u |t| + w |dd| = 2u |t|
        e' = e + t       |de'| <= u |e'| + 2u |t|          (a fused multiply-add only drops the second)"""
    e0, p = e0.astype(np.float64), p.astype(np.float64)
    want = Opt._ema_reference(e0, p, momentum)
    t = (p - e0) * float(np.float32(1.0) - np.float32(momentum))
    assert np.array_equal(want, e0 + t)
    return want, 1.001 * U * (np.abs(want) + 2 * np.abs(t))


@pytest.mark.parametrize("momentum", [0.99, 0.5])
@pytest.mark.parametrize("count", NORM_COUNTS[1:])
def test_ema_update_edges(ctx, guards, count, momentum):
    rng = np.random.default_rng(count % 1000 + 11)
    e0, p = rng.normal(0, 1, count).astype(np.float32), rng.normal(0, 1, count).astype(np.float32)
    ema = guards.out((count, 1))
    ema.upload(e0)
    d_p = guards.inp(p.reshape(count, 1))
    report = ""
    for _ in range(2):                                  # the second update starts from the device's own first
        e0 = ema.download().ravel()
        ctx.call("ssdseg_ema_update", ema, d_p, C.c_size_t(count), f32(momentum))
        want, bound = ema_bound(e0, p, f32(momentum))
        got = ema.download().ravel()
        report = assert_within("ema", got, want, bound)
        assert np.abs(got.astype(np.float64) - e0).max() > 1000 * bound.max(), "the update does not dwarf the rounding"
    print(f"\nema count={count} momentum={momentum}: {report}")
    ctx.sync()
    guards.check()


@pytest.mark.parametrize("count", NORM_COUNTS[1:])
def test_ema_update_fixed_points(ctx, guards, count):
    """ema == p stays bit-identical at any momentum; momentum 1 leaves the EMA as it is; momentum 0 gives p up to the rounding of
    the difference and of the sum, e + fl(p - e): |error| <= u (|p| + |p - e|) (the product with 1 is exact)"""
    rng = np.random.default_rng(count % 1000 + 13)
    e0, p = rng.normal(0, 1, count).astype(np.float32), rng.normal(0, 1, count).astype(np.float32)
    n = C.c_size_t(count)
    d_p = guards.inp(p.reshape(count, 1))
    ema = guards.out((count, 1))
    for momentum in (0.99, 0.5, 0.0, 1.0):
        ema.upload(p)
        ctx.call("ssdseg_ema_update", ema, d_p, n, momentum)
        assert np.array_equal(bits(ema.download().ravel()), bits(p)), f"ema == p moved at momentum {momentum}"
    ema.upload(e0)
    ctx.call("ssdseg_ema_update", ema, d_p, n, 1.0)
    assert np.array_equal(bits(ema.download().ravel()), bits(e0)), "momentum 1 changed the EMA"
    ctx.call("ssdseg_ema_update", ema, d_p, n, 0.0)
    p64, e64 = p.astype(np.float64), e0.astype(np.float64)
    print("\n" + assert_within(f"ema count={count} momentum=0", ema.download().ravel(), p64, 1.001 * U * (np.abs(p64) + np.abs(p64 - e64))))
    ctx.sync()
    guards.check()


# ------------------------------------------------------------------------------------------------------------------ the model
CLIPNORM = 1e-3


def trained_once(ctx, rng_seed, optimizer, world=1, steps=1):
    """a freshly built 96x128 model, compiled with `optimizer`, after `steps` train_steps on one seeded batch of 3 ->
    (model, engine, parameters before the first step)"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    compile_with(model, optimizer)
    (x, targets), = batches(np.random.default_rng(rng_seed), boxes, 1)
    eng = E.engine_for(model, 3, True)
    p0 = eng.P["params"].download()
    for _ in range(steps):
        eng.train_step(x, targets, optimizer=optimizer, world=world)
    ctx.sync()
    return model, eng, p0


def test_global_clipnorm_through_the_engine(ctx):
    """one train_step under SGD(momentum 0.9, weight_decay 1e-2, global_clipnorm 1e-3): the clip is live, P's norm float is the
    float64 norm of the gradient bucket within 1 ulp, parameters and velocity are the specification's with the float64 factor within
    sgd_bound widened by 2u |lr g'| (the factor's own ulp); the unclipped specification misses.  And with world=2 and no
    all-reduce -- the same gradient, grad_scale 1/2 -- the reported norm is half the single-rank one."""
    opt = Opt.SGD(momentum=0.9, weight_decay=1e-2, global_clipnorm=CLIPNORM)
    model, eng, p0 = trained_once(ctx, 1993, opt)
    P = eng.P
    g0, got_p, got_v, clip = P["grads"].download(), P["params"].download(), eng.opt.slots["velocity"].download(), eng.opt.clip.download()
    norm64, factor64 = Opt._clip_reference(g0, 1.0, f32(CLIPNORM))
    assert norm64 > CLIPNORM and factor64 < 1, "the clip is not live"
    assert ulps(clip[0], norm64) <= 1 and ulps(clip[1], factor64) <= 1, (clip, norm64, factor64)
    lr, mu = f32(0.01), f32(0.9)
    ends, lams = layer_table(model, 1e-2, ("kernel", "pointwise_kernel"))
    lam = Opt.expand_runs(ends, lams, p0.size)
    zero = np.zeros(p0.size)
    sp, sv = Opt._sgd_reference(p0.astype(np.float64), g0, zero, lr, mu, False, 1.0, ends, lams, clip_scale=factor64)
    geff = g0.astype(np.float64) * factor64
    wp, wv, bp, bv = sgd_bound(p0, geff, np.zeros_like(p0), lr, mu, False, 1.0, lam)
    assert np.allclose(sp, wp, rtol=1e-12, atol=0)
    wider = 2 * U * np.abs(lr * geff)
    print(f"\nmodel step, global_clipnorm {CLIPNORM:g}: norm {clip[0]!r}, factor {clip[1]!r}; " + assert_within("p", got_p, sp, bp + wider) + "; "
          + assert_within("v", got_v, sv, bv + wider))
    plain, _ = Opt._sgd_reference(p0.astype(np.float64), g0, zero, lr, mu, False, 1.0, ends, lams)
    assert (np.abs(got_p - plain) > bp + wider).any(), "the unclipped specification passes too"
    # the mean gradient of two ranks that hold the same gradient
    _, eng2, p0_2 = trained_once(ctx, 1993, Opt.SGD(momentum=0.9, weight_decay=1e-2, global_clipnorm=CLIPNORM), world=2)
    assert np.array_equal(bits(p0_2), bits(p0)) and np.array_equal(bits(eng2.P["grads"].download()), bits(g0)), "the twin is no twin"
    half = eng2.opt.clip.download()
    assert ulps(half[0], norm64 / 2) <= 1 and ulps(half[0], np.float32(0.5) * clip[0]) <= 1, (half, clip)
    assert ulps(half[1], Opt._clip_reference(g0, 0.5, f32(CLIPNORM))[1]) <= 1


def test_a_clip_that_never_bites_is_the_run_without_it(ctx):
    """global_clipnorm=1e30: parameters, velocity, BatchNorm state and the counter after two steps are bit-identical to a twin model
    trained without the argument on the same batch"""
    plain = trained_once(ctx, 7, Opt.SGD(momentum=0.9, weight_decay=1e-2), steps=2)[1]
    huge = trained_once(ctx, 7, Opt.SGD(momentum=0.9, weight_decay=1e-2, global_clipnorm=1e30), steps=2)[1]
    a, b = run_snapshot(ctx, plain, ("velocity",)), run_snapshot(ctx, huge, ("velocity",))
    assert a["t"] == b["t"] == 2 and plain.opt.clip is None
    clip = huge.opt.clip.download()
    assert clip[0] > CLIPNORM and clip[1] == 1.0
    for key in ("p", "s", "velocity"):
        assert np.array_equal(bits(a[key]), bits(b[key])), f"{key} differs from the run without global_clipnorm"


def test_fit_reports_grad_norm_only_with_global_clipnorm(ctx, rng):
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    data = batches(rng, boxes, 1)
    compile_with(model, Opt.SGD(momentum=0.9))
    without = model.fit(data, epochs=1)
    assert "grad_norm" not in without.history
    compile_with(model, Opt.SGD(momentum=0.9, global_clipnorm=CLIPNORM))
    hist = model.fit(data, epochs=2)
    assert set(hist.history) == set(without.history) | {"grad_norm"} and len(hist.history["grad_norm"]) == 2
    eng = E.engine_for(model, 3, True)
    norm64, _ = Opt._clip_reference(eng.P["grads"].download(), 1.0, None)
    assert ulps(hist.history["grad_norm"][-1], norm64) <= 1 and norm64 > CLIPNORM           # the pre-clip norm of the last update
    compile_with(model, Opt.SGD(momentum=0.9, clipvalue=1.0))
    assert "grad_norm" not in model.fit(data, epochs=1).history


def test_clipvalue_through_the_engine(ctx):
    """clipvalue alone, on Adam with weight decay (the engine's NULL-factor call of ssdseg_adamw_step_clipped): within adamw_bound of the
    specification.  Control: m of the unclipped specification misses on an element whose gradient exceeds the threshold (p itself
    hardly tells at update 1: m / sqrt(v) is the gradient's sign either way)."""
    value = 1e-3
    opt = Opt.Adam(learning_rate=1e-3, weight_decay=1e-2, clipvalue=value)
    model, eng, p0 = trained_once(ctx, 1993, opt)
    P = eng.P
    assert eng.opt.clip is None
    g0, got_p, got_m, got_v = (b.download() for b in (P["grads"], P["params"], eng.opt.slots["m"], eng.opt.slots["v"]))
    c = f32(value)
    over = np.abs(g0) > c
    assert 0.01 < over.mean() < 0.99, over.mean()
    lr, b1, b2, eps = f32(1e-3), f32(0.9), f32(0.999), f32(1e-7)
    ends, lams = layer_table(model, 1e-2, ("kernel", "pointwise_kernel"))
    lam = Opt.expand_runs(ends, lams, p0.size)
    zero = np.zeros(p0.size)
    spec = Opt._adamw_reference(p0.astype(np.float64), g0, zero, zero, 1, lr, b1, b2, eps, 1.0, ends, lams, clip_value=c)
    wp, wm, wv, bm, bv, bp = adamw_bound(p0, clamp64(g0.astype(np.float64), c), np.zeros_like(p0), np.zeros_like(p0), 1, lr, b1, b2, eps, 1.0, lam)
    assert all(np.allclose(a, b, rtol=1e-12, atol=0) for a, b in zip(spec, (wp, wm, wv)))
    print(f"\nmodel step, clipvalue {value:g} ({100 * over.mean():.0f} % clamped): " + assert_within("p", got_p, spec[0], bp) + "; "
          + assert_within("m", got_m, spec[1], bm) + "; " + assert_within("v", got_v, spec[2], bv))
    plain = Opt._adamw_reference(p0.astype(np.float64), g0, zero, zero, 1, lr, b1, b2, eps, 1.0, ends, lams)
    miss = np.abs(got_m - plain[1]) > bm
    # (an element a few ulps beyond the threshold stays inside the bound: most, not all)
    assert miss[over].mean() > 0.99 and not miss[~over].any(), "the unclipped specification must miss where, and only where, the gradient exceeds the threshold"


# ------------------------------------------------------------------------------------------------------------------ (f) EMA
def test_ema_through_the_engine(ctx, rng, tmp_path):
    """use_ema, ema_momentum 0.5: the average starts as the initial parameters and follows _ema_reference on its own previous value
    and the new parameters after every update; averaged_weights shows it to Model.save and gives the raw bits back, also when the
    block raises; a train_step inside raises; finalize_variable_values leaves the parameters equal to it."""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    opt = Opt.SGD(learning_rate=0.01, momentum=0.9, use_ema=True, ema_momentum=0.5)
    compile_with(model, opt)
    data = batches(rng, boxes, 3)
    eng = E.engine_for(model, 3, True)
    P, S = eng.P, eng.opt
    p0 = P["params"].download()
    before = Opt.get_state(model)[2]
    for l, w, off, size in Opt.bucket_entries(model):
        assert np.array_equal(bits(before[f"{l.name}/{w}:ema"].ravel()), bits(p0[off:off + size])), "before the first step the EMA is the parameters"
    ema_prev = p0
    for k, (x, targets) in enumerate(data):
        eng.train_step(x, targets, optimizer=opt)
        ctx.sync()
        p_new, ema = P["params"].download(), S.slots["ema"].download()
        want, bound = ema_bound(ema_prev, p_new, f32(0.5))
        print(f"\nupdate {k + 1}: " + assert_within("ema", ema, want, bound))
        assert not np.array_equal(ema, p_new) and not np.array_equal(ema, ema_prev)
        ema_prev = ema
    raw, ema = P["params"].download(), S.slots["ema"].download()
    state = P["state"].download()
    with Opt.averaged_weights(model) as m:
        assert m is model and np.array_equal(bits(P["params"].download()), bits(ema)), "inside, the bucket holds the EMA"
        model.save(str(tmp_path / "averaged"))
        with pytest.raises(RuntimeError, match="averaged_weights"):
            eng.train_step(*data[0], optimizer=opt)
        with pytest.raises(RuntimeError, match="nest"):
            with Opt.averaged_weights(model):
                pass
    assert np.array_equal(bits(P["params"].download()), bits(raw)), "the raw parameters are not back"
    saved = np.load(str(tmp_path / "averaged.npz"))
    for l, w, off, size in Opt.bucket_entries(model):
        assert np.array_equal(bits(saved[f"{l.name}/{w}"].ravel()), bits(ema[off:off + size])), f"Model.save inside the block did not write the EMA of {l.name}/{w}"
    with pytest.raises(ZeroDivisionError):
        with Opt.averaged_weights(model):
            1 / 0
    assert np.array_equal(bits(P["params"].download()), bits(raw)) and not S.averaging, "the raw parameters are not back after an exception"
    assert np.array_equal(bits(P["state"].download()), bits(state)) and np.array_equal(bits(S.slots["ema"].download()), bits(ema))
    assert S.step == 3
    eng.train_step(*data[0], optimizer=opt)              # training goes on afterwards
    ctx.sync()
    assert S.step == 4
    Opt.finalize_variable_values(model)
    assert np.array_equal(bits(P["params"].download()), bits(S.slots["ema"].download()))


def test_ema_overwrite_frequency(ctx, rng):
    """ema_overwrite_frequency=2: the parameters equal the EMA bit for bit after update 2, and not after updates 1 and 3"""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build()
    opt = Opt.SGD(learning_rate=0.01, momentum=0.9, use_ema=True, ema_momentum=0.5, ema_overwrite_frequency=2)
    compile_with(model, opt)
    eng = E.engine_for(model, 3, True)
    same = []
    for x, targets in batches(rng, boxes, 3):
        eng.train_step(x, targets, optimizer=opt)
        ctx.sync()
        same.append(bool(np.array_equal(bits(eng.P["params"].download()), bits(eng.opt.slots["ema"].download()))))
    assert same == [False, True, False]


# ------------------------------------------------------------------------------------------------------------------ (g) resume
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_resume_with_clipping_and_ema(ctx, rng, kind, tmp_path):
    """the protocol of test_resume_from_weights_and_optimizer_state with global_clipnorm, use_ema and ema_overwrite_frequency=3: four
    updates in one go == two updates, Model.save + save_state, a freshly built and compiled model, load_weights + load_state, two
    more -- parameters, BatchNorm state, the slots, the EMA and the counter bit for bit (update 3, the overwrite, lies after the
    resume).  Control: a state file's EMA replaced by zeros gives another EMA."""
    from ssdseglib import _engine as E
    E.set_default_context(ctx)

    def optimizer():
        sched = Opt.PolynomialDecay(1e-2, 4, end_learning_rate=1e-3, power=0.9)
        extra = dict(global_clipnorm=CLIPNORM, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=3)
        return Opt.Adam(learning_rate=sched, weight_decay=1e-2, **extra) if kind == "adam" else \
            Opt.SGD(learning_rate=sched, momentum=0.9, nesterov=True, weight_decay=1e-2, **extra)

    slots = (("m", "v") if kind == "adam" else ("velocity",)) + ("ema", "clip")

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
    assert want["t"] == 4 and want["clip"][1] < 1, "the clip is not live"

    _, first = fresh()
    steps(first, data[:2])
    weights, state = str(tmp_path / "weights"), str(tmp_path / "optimizer")
    first.save(weights)
    Opt.save_state(first, state)
    assert any(k.endswith(":ema") for k in np.load(state + ".npz").files)

    _, second = fresh()
    second.load_weights(weights)
    Opt.load_state(second, state)
    assert getattr(second, "_engine_params", None) is None
    got = run_snapshot(ctx, steps(second, data[2:]), slots)
    assert got["t"] == 4
    for key in want:
        if key != "t":
            assert np.array_equal(bits(got[key]), bits(want[key])), f"{key} differs after the resume"
    assert not np.array_equal(want["p"], want["ema"])

    # control: the same resume with the checkpoint's EMA zeroed
    kind_, step_, arrays = Opt.get_state(first)
    _, third = fresh()
    third.load_weights(weights)
    Opt.set_state(third, kind_, step_, {k: (np.zeros_like(a) if k.endswith(":ema") else a) for k, a in arrays.items()})
    ctrl = run_snapshot(ctx, steps(third, data[2:]), slots)
    assert ctrl["t"] == 4 and not np.array_equal(ctrl["ema"], want["ema"])
