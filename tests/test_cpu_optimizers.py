"""The optimizer surface without a GPU: the NumPy specifications of ssdseg_sgd_step / ssdseg_adamw_step against torch and against
values worked by hand, the learning-rate schedules, the weight-decay run table of the two backbones from their graphs, the
argument checks of the two entry points, and the optimizer state file."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ssdseglib import _hip
    if not os.path.exists(_hip.library_path()):
        g.build()
    return _hip.load_library()


# ------------------------------------------------------------------------------------------------------------ the specs
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_reference_equals_torch_sgd(momentum, nesterov):
    """Keras keeps v = momentum v - lr g and adds it, torch keeps b = momentum b + g and subtracts lr b: v = -lr b while the rate
    is constant, so the parameters agree to rounding (float64, 5 steps, 1e-12)"""
    import torch
    from ssdseglib import optimizers as Opt
    rng = np.random.default_rng(7)
    p = rng.normal(0, 1, 37)
    grads = rng.normal(0, 1, (5, 37))
    tp = torch.tensor(p.copy(), dtype=torch.float64, requires_grad=True)
    topt = torch.optim.SGD([tp], lr=0.05, momentum=momentum, nesterov=nesterov)
    v = np.zeros_like(p)
    for g in grads:
        p, v = Opt._sgd_reference(p, g, v, 0.05, momentum, nesterov)
        tp.grad = torch.tensor(g.copy(), dtype=torch.float64)
        topt.step()
        assert np.abs(p - tp.detach().numpy()).max() < 1e-12
    assert p.dtype == np.float64


def test_decoupled_decay_by_hand():
    """six elements, two runs: [0, 2) decays with lambda 0.5, [2, 6) does not; lr 0.1, so the decayed elements lose 5 % first"""
    from ssdseglib import optimizers as Opt
    p = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    g = np.array([1.0, -2.0, 0.0, 4.0, 0.5, 10.0])
    ends, lams = np.array([2, 6], np.int64), np.array([0.5, 0.0], np.float32)
    np.testing.assert_array_equal(Opt.expand_runs(ends, lams, 6), [0.5, 0.5, 0, 0, 0, 0])
    np.testing.assert_array_equal(Opt.expand_runs(np.array([2, 4], np.int64), np.array([0.5, 0.25], np.float32), 6), [0.5, 0.5, 0.25, 0.25, 0, 0])
    # plain: p1 = (0.95, 1.9, 3, 4, 5, 6), then - 0.1 g
    got, _ = Opt._sgd_reference(p, g, None, 0.1, run_end=ends, run_decay=lams)
    np.testing.assert_allclose(got, [0.85, 2.1, 3.0, 3.6, 4.95, 5.0], rtol=0, atol=1e-15)
    # grad_scale 0.5 halves the gradient, not the decay
    got, _ = Opt._sgd_reference(p, g, None, 0.1, grad_scale=0.5, run_end=ends, run_decay=lams)
    np.testing.assert_allclose(got, [0.9, 2.0, 3.0, 3.8, 4.975, 5.5], rtol=0, atol=1e-15)
    # momentum 0.5 from v0 = 1: v = 0.5 - 0.1 g = (0.4, 0.7, 0.5, 0.1, 0.45, -0.5); p = p1 + v
    v0 = np.ones(6)
    got, v = Opt._sgd_reference(p, g, v0, 0.1, 0.5, False, run_end=ends, run_decay=lams)
    np.testing.assert_allclose(v, [0.4, 0.7, 0.5, 0.1, 0.45, -0.5], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got, [1.35, 2.6, 3.5, 4.1, 5.45, 5.5], rtol=0, atol=1e-15)
    # Nesterov: p = p1 + 0.5 v - 0.1 g = p1 + (0.1, 0.55, 0.25, -0.35, 0.175, -1.25)
    got, v = Opt._sgd_reference(p, g, v0, 0.1, 0.5, True, run_end=ends, run_decay=lams)
    np.testing.assert_allclose(got, [1.05, 2.45, 3.25, 3.65, 5.175, 4.75], rtol=0, atol=1e-15)
    # AdamW, first step from zero moments with eps = 0: the Adam step is lr * sign(g) exactly where g != 0, so
    # p = p1 - 0.1 sign(g); the decay uses lr itself, not the bias-corrected rate
    g1 = np.array([1.0, -2.0, 3.0, 4.0, -0.5, 10.0])
    got, m, vv = Opt._adamw_reference(p, g1, np.zeros(6), np.zeros(6), 1, lr=0.1, b1=0.9, b2=0.999, eps=0.0, run_end=ends, run_decay=lams)
    np.testing.assert_allclose(got, [0.85, 2.0, 2.9, 3.9, 5.1, 5.9], rtol=0, atol=1e-14)
    np.testing.assert_allclose(m, 0.1 * g1, rtol=1e-15)
    np.testing.assert_allclose(vv, 0.001 * g1 * g1, rtol=1e-13)
    # no table: plain Adam, the oracle's formula
    from oracle import np_ops as O
    m0, v0 = np.full(6, 0.1), np.full(6, 0.02)
    want = O.adam_step(p, g1, m0, v0, 3, lr=0.1)
    for a, b in zip(Opt._adamw_reference(p, g1, m0, v0, 3, lr=0.1), want):
        np.testing.assert_allclose(a, b, rtol=1e-15)
    # dtype-generic
    got32, _ = Opt._sgd_reference(p.astype(np.float32), g.astype(np.float32), None, 0.1, run_end=ends, run_decay=lams)
    assert got32.dtype == np.float32


# ------------------------------------------------------------------------------------------------------------ schedules
def test_schedules_by_hand():
    from ssdseglib import optimizers as Opt
    pw = Opt.PiecewiseConstantDecay([10, 20], [1.0, 0.5, 0.1])
    assert [pw(s) for s in (0, 10, 11, 20, 21, 1000)] == [1.0, 1.0, 0.5, 0.5, 0.1, 0.1]
    pw = Opt.PiecewiseConstantDecay([0, 1], [1e-2, 1e-3, 1e-4])
    assert [pw(s) for s in (0, 1, 2, 3)] == [1e-2, 1e-3, 1e-4, 1e-4]
    with pytest.raises(ValueError):
        Opt.PiecewiseConstantDecay([10], [1.0])
    poly = Opt.PolynomialDecay(0.1, 100, end_learning_rate=0.01, power=2.0)
    for step, want in ((0, 0.1), (50, 0.09 * 0.25 + 0.01), (100, 0.01), (150, 0.01)):
        assert abs(poly(step) - want) < 1e-16, step
    assert Opt.PolynomialDecay(0.1, 100)(100) == 1e-4                   # Keras' default end rate
    cos = Opt.CosineDecay(0.1, 100, alpha=0.1)
    for step, want in ((0, 0.1), (50, 0.1 * (0.9 * 0.5 + 0.1)), (100, 0.01), (200, 0.01)):
        assert abs(cos(step) - want) < 1e-16, step
    warm = Opt.CosineDecay(0.0, 100, warmup_target=0.2, warmup_steps=10)
    for step, want in ((0, 0.0), (5, 0.1), (9, 0.18), (10, 0.2), (11, 0.2 * 0.5 * (1 + math.cos(math.pi * 0.01))), (60, 0.1), (110, 0.0), (500, 0.0)):
        assert abs(warm(step) - want) < 1e-16, step
    assert warm(9) < warm(10) > warm(11)
    assert Opt.rate_at(3e-4, 17) == 3e-4 and Opt.rate_at(pw, 1) == 1e-3
    assert Opt.is_schedule(pw) and not Opt.is_schedule(1e-3)


@pytest.mark.parametrize("power", [1.0, 0.9, 2.0])
def test_polynomial_decay_equals_torch_polynomial_lr(power):
    import torch
    from ssdseglib import optimizers as Opt
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.05)
    sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=10, power=power)
    ours = Opt.PolynomialDecay(0.05, 10, end_learning_rate=0.0, power=power)
    for step in range(13):
        assert abs(ours(step) - opt.param_groups[0]["lr"]) < 1e-12 * 0.05, step      # torch chains ratios: a few ulp of the base rate
        opt.step()
        sched.step()


def test_cosine_decay_equals_torch_cosine_annealing():
    import torch
    from ssdseglib import optimizers as Opt
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.05)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=10, eta_min=0.0)
    ours = Opt.CosineDecay(0.05, 10, alpha=0.0)
    for step in range(11):
        assert abs(ours(step) - opt.param_groups[0]["lr"]) < 1e-12 * 0.05, step
        opt.step()
        sched.step()


def test_optimizer_descriptions():
    from ssdseglib import optimizers as Opt
    a = Opt.Adam(learning_rate=1e-4)
    assert (a.learning_rate, a.beta_1, a.beta_2, a.epsilon, a.weight_decay) == (1e-4, 0.9, 0.999, 1e-7, 0.0)
    assert a.weight_decay_names == ("kernel", "pointwise_kernel") and a.kind == "adam" and a.slots == ("m", "v")
    s = Opt.SGD()
    assert (s.learning_rate, s.momentum, s.nesterov, s.weight_decay, s.slots) == (0.01, 0.0, False, 0.0, ())
    assert Opt.SGD(momentum=0.9).slots == ("velocity",)
    sched = Opt.PolynomialDecay(0.1, 10)
    assert Opt.SGD(learning_rate=sched).learning_rate is sched
    with pytest.raises(ValueError):
        Opt.SGD(momentum=1.0)


# ------------------------------------------------------------------------------------------------------------ run table
def mobilenet_model():
    import ssdseglib
    from ssdseglib import _graph as K
    K.set_seed(11)
    shape, fmaps = (96, 128, 3), ((6, 8), (3, 4), (2, 2), (1, 1))
    boxes = ssdseglib.boxes.DefaultBoundingBoxes(feature_maps_shapes=fmaps, centers_padding_from_borders_percentage=0.05, boxes_scales=(0.15, 0.95))
    boxes.rescale_boxes_coordinates(shape[:2])
    builder = ssdseglib.models.MobileNetV2SsdSegBuilder(
        shape, [6, 6, 6, 6], 4, boxes.get_boxes_coordinates_center_x('ssd'), boxes.get_boxes_coordinates_center_y('ssd'),
        boxes.get_boxes_coordinates_width('ssd'), boxes.get_boxes_coordinates_height('ssd'), (0.1, 0.1, 0.2, 0.2))
    return builder.get_model_for_training('deeplabv3plus', 'ssdlite', (3, 6, 12))


def shufflenet_model():
    import ssdseglib
    from ssdseglib import _graph as K
    K.set_seed(3)
    d = np.zeros(4, np.float32)
    b = ssdseglib.models.ShuffleNetV2SsdSegBuilder((96, 128, 3), '1x', True, True, 6, 4, d, d, d, d, (0.1, 0.1, 0.2, 0.2))
    return b.get_model_for_training('deeplabv3plus', 'ssdlite', (3, 6, 12))


@pytest.mark.parametrize("which", ["mobilenetv2", "shufflenetv2-1x"])
def test_run_table_from_the_model_graph(which):
    from ssdseglib import optimizers as Opt
    model = mobilenet_model() if which == "mobilenetv2" else shufflenet_model()
    opt = Opt.SGD(momentum=0.9, weight_decay=5e-4)
    ends, lams = Opt.model_decay_runs(model, opt)
    n_tr = sum(l.weights[w].size for l in model.layers for w in l.weights if w in l.trainable_names)
    assert ends.dtype == np.int64 and lams.dtype == np.float32 and ends.size == lams.size
    assert 2 < ends.size <= 4096
    assert ends[-1] == n_tr and ends[0] > 0 and (np.diff(ends) > 0).all()          # covers [0, n_tr) exactly, ascending
    assert (lams[1:] != lams[:-1]).all()                                             # adjacent equal-lambda runs are merged
    assert set(lams.tolist()) == {0.0, float(np.float32(5e-4))}
    direct = []                                                                      # layer by layer, name by name
    for l in model.layers:
        for wname, arr in l.weights.items():
            if wname in l.trainable_names:
                direct.append(np.full(arr.size, 5e-4 if wname in ("kernel", "pointwise_kernel") else 0.0, np.float32))
    direct = np.concatenate(direct)
    assert direct.size == n_tr
    np.testing.assert_array_equal(Opt.expand_runs(ends, lams, n_tr, np.float32), direct)
    seen = {w for l in model.layers for w in l.weights if w in l.trainable_names}
    assert {"kernel", "depthwise_kernel", "gamma", "beta"} <= seen
    if which == "shufflenetv2-1x":
        assert (ends[:-1] % 4 != 0).any(), "no run boundary inside a float4: the 58- / 122-channel vectors are gone?"
        assert (ends[:-1] % 4 == 2).any()
    # other names, no decay
    e2, l2 = Opt.decay_runs([(w, off, size) for _, w, off, size in Opt.bucket_entries(model)], 0.1, ("gamma",))
    assert np.array_equal(Opt.expand_runs(e2, l2, n_tr) != 0,
                          np.concatenate([np.full(l.weights[w].size, w == "gamma") for l in model.layers for w in l.weights if w in l.trainable_names]))
    e0, l0 = Opt.model_decay_runs(model, Opt.Adam())
    assert e0.size == 0 and l0.size == 0


# ------------------------------------------------------------------------------------------------------------ C-ABI
def test_optimizer_argument_errors_do_not_need_a_device(lib):
    """every check runs before the ctx or any buffer is touched (stand-ins that are never dereferenced)"""
    from ssdseglib import _hip
    header = open(os.path.join(REPO, "include", "ssdseg.h")).read()
    cap = int(re.search(r"#define\s+SSDSEG_DECAY_RUNS_MAX\s+(\d+)", header).group(1))
    assert cap >= 1024 and cap == _hip.DECAY_RUNS_MAX
    ctx, buf = C.create_string_buffer(8), C.create_string_buffer(8)
    n = C.c_size_t(4)

    def sgd(params=buf, grads=buf, velocity=buf, momentum=0.9, run_end=None, run_decay=None, nruns=0, count=n):
        return lib.ssdseg_sgd_step(ctx, params, grads, velocity, count, 0.1, momentum, 0, 1.0, run_end, run_decay, nruns)

    assert sgd(params=None) == -1000 - 2
    assert b"ssdseg_sgd_step: invalid argument 2" in lib.ssdseg_last_error()
    assert sgd(grads=None) == -1000 - 3
    assert sgd(momentum=1.0) == -1000 - 7
    assert sgd(momentum=-0.1) == -1000 - 7
    assert sgd(velocity=None) == -1000 - 4
    assert sgd(nruns=-1) == -1000 - 12
    assert sgd(nruns=1) == -1000 - 10
    assert sgd(nruns=1, run_end=buf) == -1000 - 11
    assert sgd(nruns=cap + 1, run_end=buf, run_decay=buf) == -1000 - 12
    assert b"ssdseg_sgd_step: invalid argument 12" in lib.ssdseg_last_error()
    assert lib.ssdseg_sgd_step(None, buf, buf, buf, n, 0.1, 0.9, 0, 1.0, None, None, 0) == -1000 - 1
    # what passes the checks: an empty bucket returns before the ctx is used -- plain SGD without a velocity, a table at the cap
    assert sgd(velocity=None, momentum=0.0, count=C.c_size_t(0)) == 0
    assert sgd(nruns=cap, run_end=buf, run_decay=buf, count=C.c_size_t(0)) == 0

    def adamw(params=buf, step=1, run_end=None, run_decay=None, nruns=0, count=n):
        return lib.ssdseg_adamw_step(ctx, params, buf, buf, buf, count, 1e-3, 0.9, 0.999, 1e-7, step, 1.0, run_end, run_decay, nruns)

    assert adamw(params=None) == -1000 - 2
    assert adamw(step=0) == -1000 - 11
    assert adamw(nruns=-1) == -1000 - 15
    assert adamw(nruns=1) == -1000 - 13
    assert adamw(nruns=1, run_end=buf) == -1000 - 14
    assert adamw(nruns=cap + 1, run_end=buf, run_decay=buf) == -1000 - 15
    assert b"ssdseg_adamw_step: invalid argument 15" in lib.ssdseg_last_error()
    assert adamw(nruns=cap, run_end=buf, run_decay=buf, count=C.c_size_t(0)) == 0


# ------------------------------------------------------------------------------------------------------------ state file
def test_optimizer_state_file_round_trip(tmp_path):
    from ssdseglib import optimizers as Opt
    rng = np.random.default_rng(3)
    model = mobilenet_model()
    entries = Opt.bucket_entries(model)
    names = [f"{l.name}/{w}" for l, w, _, _ in entries]
    assert len(set(names)) == len(names) > 100
    shapes = {f"{l.name}/{w}": l.weights[w].shape for l, w, _, _ in entries}
    path = str(tmp_path / "opt")

    with pytest.raises(ValueError, match="compiled optimizer"):
        Opt.save_state(model, path)
    model.compile(optimizer=Opt.SGD(learning_rate=0.1, momentum=0.9))
    kind, step, arrays = Opt.get_state(model)                       # before any step: the initial state
    assert (kind, step) == ("sgd", 0) and set(arrays) == {k + ":velocity" for k in names} and not any(a.any() for a in arrays.values())

    placed = {k + ":velocity": rng.normal(0, 1, s).astype(np.float32) for k, s in shapes.items()}
    Opt.set_state(model, "sgd", 41, placed)
    Opt.save_state(model, path)
    data = np.load(path + ".npz")
    assert int(data["step"]) == 41 and str(data["kind"]) == "sgd" and set(data.files) == set(placed) | {"step", "kind"}
    weights_keys = set()
    for l in model.layers:
        weights_keys |= {f"{l.name}/{w}" for w in l.weights}
    assert {k.rsplit(":", 1)[0] for k in placed} <= weights_keys              # Model.save's keys

    def fresh(optimizer):
        m = mobilenet_model()       # the same seed and builder: the same layer names
        m.compile(optimizer=optimizer)
        return m

    other = fresh(Opt.SGD(learning_rate=0.1, momentum=0.9))
    Opt.load_state(other, path)
    kind, step, arrays = Opt.get_state(other)
    assert (kind, step) == ("sgd", 41) and set(arrays) == set(placed)
    for k, a in placed.items():
        assert arrays[k].dtype == np.float32 and np.array_equal(arrays[k], a), k

    with pytest.raises(ValueError, match="kind"):
        Opt.load_state(fresh(Opt.Adam()), path)
    victim = sorted(placed)[5]
    broken = dict(placed)
    del broken[victim]
    np.savez(str(tmp_path / "missing.npz"), step=np.int64(41), kind=np.asarray("sgd"), **broken)
    with pytest.raises(KeyError, match=re.escape(victim)):
        Opt.load_state(fresh(Opt.SGD(momentum=0.9)), str(tmp_path / "missing"))
    broken = dict(placed)
    broken[victim] = np.zeros(placed[victim].shape + (2,), np.float32)
    np.savez(str(tmp_path / "shape.npz"), step=np.int64(41), kind=np.asarray("sgd"), **broken)
    with pytest.raises(ValueError, match="shape"):
        Opt.load_state(fresh(Opt.SGD(momentum=0.9)), str(tmp_path / "shape"))
    # Adam: two arrays per weight
    adam = fresh(Opt.Adam())
    placed = {f"{k}:{s}": rng.normal(0, 1, shp).astype(np.float32) for k, shp in shapes.items() for s in ("m", "v")}
    Opt.set_state(adam, "adam", 7, placed)
    Opt.save_state(adam, str(tmp_path / "adam.npz"))
    again = fresh(Opt.Adam(weight_decay=1e-2))
    Opt.load_state(again, str(tmp_path / "adam.npz"))
    kind, step, arrays = Opt.get_state(again)
    assert (kind, step) == ("adam", 7) and all(np.array_equal(arrays[k], a) for k, a in placed.items())


# ------------------------------------------------------------------------------------------------------------ imports
def test_optimizers_imports_neither_the_engine_nor_the_state_object():
    """in a fresh interpreter `import ssdseglib.optimizers` succeeds and loads neither ssdseglib._engine nor ssdseglib._optim:
    descriptions, schedules, specifications and the checkpoint reach the device-side state through the model only"""
    import subprocess
    import sys
    import ssdseglib
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(ssdseglib.__file__)))
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import ssdseglib.optimizers; "
            "print(sorted(m for m in ('ssdseglib._engine', 'ssdseglib._optim') if m in sys.modules))")
    r = subprocess.run([sys.executable, "-c", code, pkg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.decode().strip() == "[]"
