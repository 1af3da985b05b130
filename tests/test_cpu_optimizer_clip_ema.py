"""Gradient clipping and EMA weights without a device: the optimizer descriptions' new arguments, the NumPy specifications
(ssdseglib.optimizers._clip_reference / _ema_reference and the clip arguments of the two step references), the `:ema` slot of the
optimizer state, and the argument errors of the four new C entries."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from tests.test_cpu_optimizers import lib, mobilenet_model  # noqa: F401  (lib: fixture)


# ------------------------------------------------------------------------------------------------------------ descriptions
@pytest.mark.parametrize("cls", ["Adam", "SGD"])
def test_constructor_validation(cls):
    from ssdseglib import optimizers as Opt
    make = getattr(Opt, cls)
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="global_clipnorm"):
            make(global_clipnorm=bad)
        with pytest.raises(ValueError, match="clipvalue"):
            make(clipvalue=bad)
    with pytest.raises(ValueError, match="at most one"):
        make(global_clipnorm=1.0, clipvalue=0.5)
    with pytest.raises(NotImplementedError, match="global_clipnorm"):
        make(clipnorm=1.0)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="ema_momentum"):
            make(use_ema=True, ema_momentum=bad)
    for bad in (0, -2, 1.5, "3", True):
        with pytest.raises(ValueError, match="ema_overwrite_frequency"):
            make(use_ema=True, ema_overwrite_frequency=bad)
    o = make(global_clipnorm=2, use_ema=True, ema_momentum=0, ema_overwrite_frequency=np.int64(3))
    assert (o.global_clipnorm, o.clipvalue, o.use_ema, o.ema_momentum, o.ema_overwrite_frequency) == (2.0, None, True, 0.0, 3)
    assert type(o.ema_overwrite_frequency) is int and make(ema_momentum=1).ema_momentum == 1.0
    assert make(clipvalue=0.5).clipvalue == 0.5 and make(clipvalue=math.inf).clipvalue == math.inf


def test_defaults_leave_the_descriptions_as_they_were():
    from ssdseglib import optimizers as Opt
    a, s = Opt.Adam(), Opt.SGD(momentum=0.9)
    for o in (a, s):
        assert (o.global_clipnorm, o.clipvalue, o.use_ema, o.ema_momentum, o.ema_overwrite_frequency) == (None, None, False, 0.99, None)
        assert Opt.state_slots(o) == tuple(o.slots)
    assert (a.learning_rate, a.beta_1, a.beta_2, a.epsilon, a.weight_decay, a.kind, a.slots) == (1e-3, 0.9, 0.999, 1e-7, 0.0, "adam", ("m", "v"))
    assert (s.learning_rate, s.momentum, s.nesterov, s.weight_decay, s.kind, s.slots) == (0.01, 0.9, False, 0.0, "sgd", ("velocity",))
    assert a.weight_decay_names == s.weight_decay_names == ("kernel", "pointwise_kernel")
    assert Opt.state_slots(Opt.SGD(use_ema=True)) == ("ema",) and Opt.state_slots(Opt.Adam(use_ema=True)) == ("m", "v", "ema")


# ------------------------------------------------------------------------------------------------------------ specifications
def test_clip_reference_by_hand():
    from ssdseglib import optimizers as Opt
    g = np.asarray([3.0, -4.0, 0.0, 12.0], np.float32)                 # norm 13
    assert Opt._clip_reference(np.zeros(7, np.float32), 1.0, 1.0) == (0.0, 1.0)               # zero gradient: no 0/0
    assert Opt._clip_reference(np.zeros(0, np.float32), 1.0, 1.0) == (0.0, 1.0)
    assert Opt._clip_reference(g, 1.0, 26.0) == (13.0, 1.0)                                   # below
    assert Opt._clip_reference(g, 1.0, 13.0) == (13.0, 1.0)                                   # equal: not clipped
    assert Opt._clip_reference(g, 1.0, 6.5) == (13.0, 0.5)                                    # above
    assert Opt._clip_reference(g, 0.5, 6.5) == (6.5, 1.0)                                     # the norm of the SCALED gradient
    assert Opt._clip_reference(g, -0.5, 3.25) == (6.5, 0.5)
    assert Opt._clip_reference(g.reshape(2, 2), 1.0, 6.5) == (13.0, 0.5)
    for off in (None, 0.0, -1.0, math.inf, math.nan):
        assert Opt._clip_reference(g, 1.0, off) == (13.0, 1.0)
    norm, factor = Opt._clip_reference(np.asarray([1.0, math.nan], np.float32), 1.0, 0.5)
    assert math.isnan(norm) and factor == 1.0                                                 # a NaN norm fails the comparison
    # squares in float64: neither overflow nor underflow where float32 would
    norm, factor = Opt._clip_reference(np.asarray([1e30] + [1e-30] * 3, np.float32), 1.0, 1.0)
    assert norm == pytest.approx(1e30, rel=1e-6) and factor == pytest.approx(1e-30, rel=1e-6)
    norm, _ = Opt._clip_reference(np.full(4, 1e-30, np.float32), 1.0, 1.0)
    assert norm == pytest.approx(2e-30, rel=1e-6)


def test_ema_reference_by_hand():
    from ssdseglib import optimizers as Opt
    e, p = np.asarray([1.0, -2.0, 0.5]), np.asarray([3.0, -2.0, 0.0])
    assert np.array_equal(Opt._ema_reference(e, p, 0.5), [2.0, -2.0, 0.25])
    assert np.array_equal(Opt._ema_reference(e, p, 1.0), e) and np.array_equal(Opt._ema_reference(e, p, 0.0), p)
    omm = float(np.float32(1) - np.float32(0.99))                      # 1 - momentum is formed in float32
    assert np.array_equal(Opt._ema_reference(e, p, 0.99), e + (p - e) * omm)
    rng = np.random.default_rng(5)
    same = rng.normal(0, 1, 1000).astype(np.float32)
    out = Opt._ema_reference(same, same.copy(), 0.99)                  # ema == p is a fixed point, bit for bit
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), same.view(np.uint32))


def test_step_references_with_default_clip_arguments_are_the_present_ones():
    """a restatement of the references as they stood before the clip arguments, compared bit for bit in float32 and float64"""
    from ssdseglib import optimizers as Opt
    rng = np.random.default_rng(1993)
    n = 257
    ends, lams = np.asarray([100, 200, n], np.int64), np.asarray([0.5, 0.0, 0.25], np.float32)
    for dt in (np.float32, np.float64):
        p, g, m, v = (rng.normal(0, 1, n).astype(dt) for _ in range(4))
        v = np.abs(v) * dt(0.01)
        lam = Opt.expand_runs(ends, lams, n, dt)
        lr, gs, mu = 0.05, 1.0 / 3.0, 0.9
        gk = g * dt(gs)
        p1 = p - (dt(lr) * lam) * p
        v1 = dt(mu) * m - dt(lr) * gk
        for nesterov, want in ((False, p1 + v1), (True, p1 + (dt(mu) * v1 - dt(lr) * gk))):
            got_p, got_v = Opt._sgd_reference(p, g, m, lr, mu, nesterov, gs, ends, lams)
            assert got_p.dtype == dt and got_p.tobytes() == want.tobytes() and got_v.tobytes() == v1.tobytes()
        got_p, got_v = Opt._sgd_reference(p, g, None, lr, 0.0, False, gs, ends, lams)
        assert got_v is None and got_p.tobytes() == (p1 - dt(lr) * gk).tobytes()
        b1, b2, eps, t = 0.9, 0.999, 1e-7, 7
        m1 = m + (gk - m) * dt(1.0 - b1)
        v2 = v + (gk * gk - v) * dt(1.0 - b2)
        alpha = dt(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
        got = Opt._adamw_reference(p, g, m, v, t, lr, b1, b2, eps, gs, ends, lams)
        for a, b in zip(got, (p1 - alpha * m1 / (np.sqrt(v2) + dt(eps)), m1, v2)):
            assert a.dtype == dt and a.tobytes() == b.tobytes()
        # and what the clip arguments do: the factor, then the clamp, NaN passing through
        g[3] = np.nan
        got_p, _ = Opt._sgd_reference(p, g, None, lr, 0.0, False, 0.5, None, None, clip_scale=0.25, clip_value=0.1)
        gc = np.clip(g * dt(0.5) * dt(0.25), -dt(0.1), dt(0.1))
        assert np.isnan(got_p[3]) and (np.abs(gc[~np.isnan(gc)]) == dt(0.1)).sum() > 10
        assert got_p.tobytes() == (p - dt(lr) * gc).tobytes()
        g[3] = 0
        got = Opt._adamw_reference(p, g, m, v, t, lr, b1, b2, eps, 1.0, None, None, clip_scale=0.25, clip_value=0.1)
        want = Opt._adamw_reference(p, np.clip(g * dt(0.25), -dt(0.1), dt(0.1)), m, v, t, lr, b1, b2, eps)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------------------ state
def test_ema_slot_of_the_optimizer_state(tmp_path):
    from ssdseglib import optimizers as Opt
    rng = np.random.default_rng(4)
    model = mobilenet_model()
    entries = Opt.bucket_entries(model)
    names = [f"{l.name}/{w}" for l, w, _, _ in entries]
    shapes = {f"{l.name}/{w}": l.weights[w].shape for l, w, _, _ in entries}

    model.compile(optimizer=Opt.SGD(momentum=0.9))
    assert set(Opt.get_state(model)[2]) == {k + ":velocity" for k in names}                   # absent without use_ema
    model.compile(optimizer=Opt.SGD(momentum=0.9, use_ema=True))
    kind, step, arrays = Opt.get_state(model)                        # before any step: zeros, and the average is the weights
    assert (kind, step) == ("sgd", 0) and set(arrays) == {k + s for k in names for s in (":velocity", ":ema")}
    for l, w, _, _ in entries:
        assert np.array_equal(arrays[f"{l.name}/{w}:ema"], l.weights[w]) and not arrays[f"{l.name}/{w}:velocity"].any()

    placed = {k + s: rng.normal(0, 1, shape).astype(np.float32) for k, shape in shapes.items() for s in (":velocity", ":ema")}
    Opt.set_state(model, "sgd", 9, placed)
    path = str(tmp_path / "opt")
    Opt.save_state(model, path)

    def fresh(optimizer):
        m = mobilenet_model()
        m.compile(optimizer=optimizer)
        return m

    other = fresh(Opt.SGD(momentum=0.9, use_ema=True, ema_overwrite_frequency=3))
    Opt.load_state(other, path)
    kind, step, arrays = Opt.get_state(other)
    assert (kind, step) == ("sgd", 9) and set(arrays) == set(placed)
    assert all(np.array_equal(arrays[k], a) for k, a in placed.items())
    # an optimizer without EMA takes the same file and leaves the slot behind
    plain = fresh(Opt.SGD(momentum=0.9))
    Opt.load_state(plain, path)
    assert set(Opt.get_state(plain)[2]) == {k + ":velocity" for k in names}
    # a file without the slot, a single missing key, a wrong shape
    without = {k: a for k, a in placed.items() if k.endswith(":velocity")}
    np.savez(str(tmp_path / "without.npz"), step=np.int64(9), kind=np.asarray("sgd"), **without)
    with pytest.raises(KeyError, match=":ema"):
        Opt.load_state(fresh(Opt.SGD(momentum=0.9, use_ema=True)), str(tmp_path / "without"))
    victim = sorted(k for k in placed if k.endswith(":ema"))[5]
    with pytest.raises(KeyError, match=re.escape(victim)):
        Opt.set_state(fresh(Opt.Adam(use_ema=True)), "adam", 1, {**{k.replace(":velocity", ":m"): a for k, a in placed.items() if k != victim},
                                                                  **{k.replace(":velocity", ":v"): a for k, a in without.items()}})
    broken = dict(placed)
    broken[victim] = np.zeros(broken[victim].shape + (2,), np.float32)
    with pytest.raises(ValueError, match="shape"):
        Opt.set_state(fresh(Opt.SGD(momentum=0.9, use_ema=True)), "sgd", 9, broken)
    # the helpers ask for an optimizer that averages
    with pytest.raises(ValueError, match="use_ema"):
        Opt.finalize_variable_values(plain)
    with pytest.raises(ValueError, match="use_ema"):
        with Opt.averaged_weights(plain):
            pass


# ------------------------------------------------------------------------------------------------------------ C-ABI
def test_clip_and_ema_argument_errors_do_not_need_a_device(lib):  # noqa: F811
    """every check runs before the ctx or any buffer is touched (stand-ins that are never dereferenced)"""
    from ssdseglib import _hip
    ctx, buf = C.create_string_buffer(8), C.create_string_buffer(8)
    n, inf, nan = C.c_size_t(4), math.inf, math.nan
    cap = _hip.DECAY_RUNS_MAX

    # the partials: a function of the count alone -- decay_blocks of the step kernels
    parts = lib.ssdseg_grad_norm_parts
    def decay_blocks(n4):          # csrc/decay_runs.h
        blocks = min(max((n4 + 255) // 256, 1), 2048)
        chunk = ((n4 + blocks - 1) // blocks + 255) // 256 * 256
        return (n4 + chunk - 1) // chunk if chunk else 1

    for c in (0, 1, 3, 4, 5, 1024, 1028, 1031, 4 * 256 * 5, 4 * 256 * 5 + 4, 10 ** 6, 10 ** 7):
        assert parts(c) == decay_blocks(c // 4) >= 1, c
    assert [parts(c) for c in (0, 3, 1024, 1028, 4 * 256 * 5)] == [1, 1, 1, 2, 5]
    grid = 2048 * 256 * 4
    assert parts(grid) == 2048 and parts(grid + 6) == 1025 and parts(4009920) == 1958 and parts(1 << 33) == 2048

    def norm(c=ctx, grads=buf, count=n, partials=buf, out=buf):
        return lib.ssdseg_grad_norm(c, grads, count, 1.0, 1.0, partials, out)

    assert norm(c=None) == -1000 - 1
    assert norm(grads=None) == -1000 - 2
    assert b"ssdseg_grad_norm: invalid argument 2" in lib.ssdseg_last_error()
    assert norm(partials=None) == -1000 - 6
    assert norm(out=None) == -1000 - 7
    assert norm(out=None, grads=None, partials=None, count=C.c_size_t(0)) == -1000 - 7          # an empty bucket still writes {0, 1}

    def sgd(params=buf, grads=buf, velocity=buf, momentum=0.9, run_end=None, run_decay=None, nruns=0, count=n, scale=buf, value=inf, c=ctx):
        return lib.ssdseg_sgd_step_clipped(c, params, grads, velocity, count, 0.1, momentum, 0, 1.0, run_end, run_decay, nruns, scale, value)

    assert sgd(c=None) == -1000 - 1
    assert sgd(params=None) == -1000 - 2
    assert sgd(grads=None) == -1000 - 3
    assert sgd(momentum=1.0) == -1000 - 7
    assert sgd(velocity=None) == -1000 - 4
    assert sgd(nruns=-1) == -1000 - 12
    assert sgd(nruns=1) == -1000 - 10
    assert sgd(nruns=1, run_end=buf) == -1000 - 11
    assert sgd(nruns=cap + 1, run_end=buf, run_decay=buf) == -1000 - 12
    for bad in (0.0, -1.0, -inf, nan):
        assert sgd(value=bad) == -1000 - 14
    assert b"ssdseg_sgd_step_clipped: invalid argument 14" in lib.ssdseg_last_error()
    for ok in (inf, 1e-30, 3.0):                                       # an empty bucket returns before the ctx is used
        assert sgd(value=ok, scale=None, velocity=None, momentum=0.0, count=C.c_size_t(0)) == 0

    def adamw(params=buf, step=1, run_end=None, run_decay=None, nruns=0, count=n, scale=buf, value=inf, c=ctx):
        return lib.ssdseg_adamw_step_clipped(c, params, buf, buf, buf, count, 1e-3, 0.9, 0.999, 1e-7, step, 1.0, run_end, run_decay, nruns, scale, value)

    assert adamw(c=None) == -1000 - 1
    assert adamw(params=None) == -1000 - 2
    assert adamw(step=0) == -1000 - 11
    assert adamw(nruns=-1) == -1000 - 15
    assert adamw(nruns=1) == -1000 - 13
    assert adamw(nruns=1, run_end=buf) == -1000 - 14
    assert adamw(nruns=cap + 1, run_end=buf, run_decay=buf) == -1000 - 15
    for bad in (0.0, -1.0, nan):
        assert adamw(value=bad) == -1000 - 17
    assert b"ssdseg_adamw_step_clipped: invalid argument 17" in lib.ssdseg_last_error()
    assert adamw(scale=None, nruns=cap, run_end=buf, run_decay=buf, count=C.c_size_t(0)) == 0

    def ema(c=ctx, e=buf, p=buf, count=n, momentum=0.99):
        return lib.ssdseg_ema_update(c, e, p, count, momentum)

    assert ema(c=None) == -1000 - 1
    assert ema(e=None) == -1000 - 2
    assert ema(p=None) == -1000 - 3
    for bad in (-0.01, 1.01, nan, inf):
        assert ema(momentum=bad) == -1000 - 5
    assert b"ssdseg_ema_update: invalid argument 5" in lib.ssdseg_last_error()
    for ok in (0.0, 1.0, 0.5):
        assert ema(momentum=ok, count=C.c_size_t(0)) == 0
