"""GPU parity of the stem conv and the 3x3 / 2 max-pool at their edges (through the C-ABI) vs float64.

ssdseg_stem_conv_parts / _fwd / _bwd_weight (csrc/stem.hip: stem_fwd_direct_kernel<Q>; the LD == 2 loader of gemm_rowA_kernel in
csrc/gemm.hip; the stem gather of gemm_wgrad_kernel in csrc/pw_wgrad.hip) and ssdseg_maxpool3x3s2_fwd / _bwd (csrc/shuffle.hip, both
backward forms) on the cases of tests/_stem_cases.py: all sixteen instantiations of the direct kernel on two images, with statistics, with
bias and with neither; every pad pair from one pixel up in both forward forms; the second pixel of a thread absent, present and a second
trip at the four values of pixels-per-block; 2,050 output rows on 2,048 blocks; the statistics table's written rows and its cleared tail
in both forms; the implicit GEMM at ragged row tiles, three images in one tile, one to six 32-wide column tiles, the 96- and 160-wide
tiles it takes from 65,536 rows and a block that walks three row tiles; the weight gradient at one step, partial steps, two and three splits with a short last one, wn = 1, 2, 3 and two column tiles, in
both gradient views; the pool at every (h, w) up to 5 x 5 and three channel counts under three views.  SSDSEG_STEM_DIRECT and
SSDSEG_MAXPOOL_BWD are set per call with monkeypatch, every pointwise switch cleared first.  tests/test_cpu_stem_cases.py vets the
reference, the cases and the mirror.  Every buffer is guarded (tests/_guard.py); the launches are read from the timing registry and the
kernel a case is there for must be among them.

Bounds.  U = 2^-24, gamma(L) = L U / (1 - L U).

  lattice family   0 for y in both forms, the float64 fold of the statistics rows to sum y, dW and dbias: pixels are integers, weights
                   multiples of 1/8, the rescale a power-of-two pair, so w . scale, offset . sum_c w, the nine-tap sum, the border
                   subtraction, fmaf(x, scale, offset) and every product are float32 numbers and every reduction stays below 2^24 units
                   of its lattice (_stem_cases.budget).  Both forward forms must give the same numbers: bit for bit after x + 0.
                   sum y^2: 0 where its budget holds too, else gamma(M + 2) sum y^2, M = n ho wo.
  pool             0 everywhere: a maximum and a routed copy round nothing; the view's fused multiply-add is exact on the lattice.
  normal family    any-order bounds on random bytes, N(0, 0.3) weights, the production rescale.
                   Direct forward (csrc/stem.hip): a term is formed with at most c2 = 3 roundings -- ws = w . scale is one (:51); an
                   offset term is sum_c w (three additions from 0, the first exact: two, :52) times offset (one, :54).  The terms
                   are then summed in one chain: wo_all over nine taps (eight roundings, :56), bias + wo_all (one, :96), up to eight
                   subtractions of the padded taps' terms (:102), 27 fused multiply-adds (:107): c1 = 8 + 1 + 8 = 17.  So
                       |dy| <= (gamma(27 + c1) + c2 U) (1 + 2^-16) T
                   with T the sum of the absolute terms the kernel forms: sum |x s w| over the valid taps (a padded tap reads 0),
                   |o| sum_c |w| over ALL nine taps, |o| sum_c |w| over the removed taps AGAIN, and |b|; 1 + 2^-16 covers the
                   products of two errors (44 . 3 U^2 against 47 U).  Contraction of :54 into :56 only removes a rounding.
                   GEMM forward: fmaf(x, s, o) rounds once per element, then 27 exact products summed in any order plus the bias:
                       (gamma(27 + 1) + U) sum (|x s| + |o|) |w| + U |b|.
                   Weight gradient: the rows of gemm_wgrad_kernel in tests/test_gpu_pw_edges.py with A = |x s| + |o| at the valid taps
                   (a padded tap is 0), D = |g| or |s g| + |k1 y| + |k0|: (gamma(M + 2) + 3 U) sum A D + U |dW|.
                   Statistics: gamma(M + 1) sum |y| + sum b; gamma(M + 2) sum y^2 + sum (2 |y| b + b^2).  dbias (ssdseg_channel_stats,
                   ssdseg_colsum): gamma(M + 1) sum |g| + U |dbias|.

Not here: the switch to the GEMM form at n h w 12 >= 2^31 needs a 2 GB batch; it is held by reading csrc/stem.hip:202.  The pool's
grid-stride second trip is run by tests/test_gpu_shufflenet_baseline.py.

Run with -s for the largest error / bound ratio of every case (DESIGN.md records them).
"""
import ctypes as C
import re

import numpy as np
import pytest

import _stem_cases as P
from oracle import np_ops as O
from _guard import BODY_WORD, guards  # noqa: F401  (fixture)
from _edge_helpers import launched, ratio, rejected, reporter, same_bits, untouched

pytestmark = pytest.mark.gpu

F32 = np.float32
report = reporter("stem-edges")
RECORDED = set()        # every kernel symbol the timing registry showed in this process
RAN = set()             # the lattice cases that ran in this process
FWD_CASES = [nm for nm, c in P.CASES.items() if c["fwd"]]
WGRAD_CASES = [nm for nm, c in P.CASES.items() if c["wgrad"]]


@pytest.fixture(scope="module")
def cus(ctx):
    """the device's CU count (the split rule of the weight gradient is sized by it) as the library itself holds it:
    ssdseg_ctx_device_name ends in "N CUs)" """
    count = re.search(r"(\d+) CUs\)$", ctx.device_name())
    assert count and int(count.group(1)) > 0, ctx.device_name()
    return int(count.group(1))


def use(monkeypatch, env):
    for v in P.STEM_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, value in env.items():
        monkeypatch.setenv(v, value)
    return env


def poisoned(a):
    return int((np.ascontiguousarray(a).view(np.uint32) == np.uint32(BODY_WORD)).sum())


def run(ctx, fn, *patterns):
    """the launches of fn(): every kernel the case is there for is among them"""
    kernels = launched(ctx, fn)
    RECORDED.update(kernels)
    for pattern in patterns:
        assert P.reaches(kernels, pattern), ("launched", kernels, "expected one matching", pattern)
    return kernels


class Dev:
    """the operands of one stem case on the device, guarded; allocated when first used"""

    def __init__(self, ctx, guards, k):
        self.ctx, self.guards, self.k = ctx, guards, k
        self._bufs = {}

    def buf(self, name):
        if name not in self._bufs:
            k, g = self.k, self.guards
            n, h, w, cout = k.shape
            m = n * k.geo[0] * k.geo[1]
            if name == "y":
                b = g.out((m, cout), name=name)
            elif name == "dW":
                b = g.out((3, 3, 3, cout), name=name)
            elif name == "dbias":
                b = g.out((cout,), name=name)
            elif name == "stats":
                rows = self.ctx.parts("ssdseg_stem_conv_parts", n, h, w, cout)
                assert rows == P.table_rows(n, h, w, cout)
                b = g.out((rows, 2, cout), name=name)
            else:
                b = g.inp(getattr(k, name), name=name)
            self._bufs[name] = b
        return self._bufs[name]

    def gview(self, gview):
        from ssdseglib import _hip as H
        if gview == "identity":
            return H.gview(self.buf("g"))
        return H.gview(self.buf("g"), self.buf("yraw"), self.buf("gscale"), self.buf("gshift"), self.buf("k1"), self.buf("k0"), act=gview)

    def fresh(self, *names):
        out = [self.guards.repoison(self.buf(nm)) for nm in names]
        return out if len(out) > 1 else out[0]


def fwd(ctx, dev, env, pair, variant):
    """-> (y, the statistics table's rows of this launch folded in float64, or None)"""
    k = dev.k
    n, h, w, cout = k.shape
    form = "gemm" if env else "direct"
    y, table = dev.fresh("y", "stats")
    bias, stats = (dev.buf("b") if variant == "bias" else None), (table if variant == "stats" else None)
    run(ctx, lambda: ctx.call("ssdseg_stem_conv_fwd", dev.buf("x"), dev.buf("w"), bias, y, n, h, w, 3, cout, pair[0], pair[1], stats),
        P.fwd_kernel(form, n, h, w, cout))
    out = y.download().reshape(n, k.geo[0], k.geo[1], cout)
    assert poisoned(out) == 0, "y is not fully written"
    if stats is None:
        assert untouched(table) == table.size
        return out, None
    t = table.download()
    mine = P.launch_rows(env, n, h, w, cout)
    assert poisoned(t[:mine]) == 0 and np.isfinite(t[:mine]).all(), "a row of the launch's statistics rows was not written"
    assert not t[mine:].view(np.uint32).any(), "a row of the statistics table beyond the launch's own is not exactly 0"
    return out, t.astype(np.float64).sum(axis=0)


def bwd_weight(ctx, dev, pair, gview, with_dbias, plan):
    k = dev.k
    n, h, w, cout = k.shape
    dw, db = dev.fresh("dW", "dbias")
    kernels = run(ctx, lambda: ctx.call("ssdseg_stem_conv_bwd_weight", dev.buf("x"), dev.gview(gview), dw, db if with_dbias else None, n, h, w, 3, cout,
                                        pair[0], pair[1]), "^" + re.escape(plan["symbol"]) + "$")
    if with_dbias:
        assert kernels.get("colsum_kernel") == (2 if plan["splits"] > 1 else 1), (kernels, plan)
    else:
        assert ("colsum_kernel" in kernels) == (plan["splits"] > 1), (kernels, plan)
        assert untouched(db) == db.size
    out = dw.download()
    assert poisoned(out) == 0, "dW is not fully written"
    dbias = db.download() if with_dbias else None
    assert dbias is None or poisoned(dbias) == 0
    return out, dbias


# ------------------------------------------------------------------------------------------------------- lattice: bound 0
@pytest.mark.parametrize("name", FWD_CASES)
def test_lattice_forward_is_exact_in_every_form(ctx, guards, monkeypatch, name):
    """every rescale pair and variant of the case under every form it names: the kernel the form is there for ran; y equals the float64
    reference (bound 0) and the other form bit for bit; the statistics rows of the launch hold no poison and fold to sum y exactly (sum
    y^2 exactly where its budget holds), the rows beyond them are exactly 0; without statistics the table keeps its poison"""
    k = P.lattice_case(name)
    case = P.CASES[name]
    n, h, w, cout = k.shape
    m = P.m_of(name)
    dev = Dev(ctx, guards, k)
    worst, first = 0.0, {}
    for form in case["forms"]:
        env = use(monkeypatch, P.FORM_ENV[form])
        for i in case["pairs"]:
            pair = P.PAIRS[i]
            sumsq_exact = P.budget(k, pair)["sumsq"] < P.EXACT
            for variant in case["variants"]:
                what = (form, pair, variant)
                y_ref = P.ref_fwd(k, pair, variant == "bias")
                y, fold = fwd(ctx, dev, env, pair, variant)
                assert ratio(y, y_ref, 0.0) == 0.0, what
                kept = first.setdefault((i, variant), (form, y + F32(0)))
                assert same_bits(y + F32(0), kept[1]), (what, "differs in bits from", kept[0])
                if fold is not None:
                    assert ratio(fold[0], y_ref.sum(axis=(0, 1, 2)), 0.0) == 0.0, (what, "the fold of the statistics rows is not sum y")
                    q_ref = (y_ref * y_ref).sum(axis=(0, 1, 2))
                    worst = max(worst, ratio(fold[1], q_ref, 0.0 if sumsq_exact else P.gamma(m + 2) * q_ref + 1e-300))
    ctx.sync()
    guards.check()
    RAN.add(name)
    report("stem-fwd", f"{name} [{k.mode}]", sumsq=worst)


@pytest.mark.parametrize("name", WGRAD_CASES)
def test_lattice_weight_gradient_is_exact(ctx, guards, monkeypatch, cus, name):
    """identity gradient view with dbias, BatchNorm gradient view (ReLU6, thresholds hit) without: the kernel the mirror names ran, the
    split partials were folded by colsum_kernel exactly when the mirror gives more than one split; dW and dbias equal the float64
    reference (bound 0)"""
    k = P.lattice_case(name)
    use(monkeypatch, {})
    dev = Dev(ctx, guards, k)
    plan = P.wgrad_plan(P.m_of(name), k.shape[3], cus)
    for i in P.CASES[name]["pairs"]:
        for gview, with_dbias in P.WGRAD_FORMS:
            dw_ref, db_ref = P.ref_bwd(k, P.PAIRS[i], gview)
            dw, db = bwd_weight(ctx, dev, P.PAIRS[i], gview, with_dbias, plan)
            assert ratio(dw, dw_ref, 0.0) == 0.0, (P.PAIRS[i], gview)
            assert db is None or ratio(db, db_ref, 0.0) == 0.0, (P.PAIRS[i], "dbias")
    ctx.sync()
    guards.check()
    RAN.add(name)


# ------------------------------------------------------------------------------------------------ normal: derived bounds
@pytest.mark.parametrize("name", P.NORMAL_CASES)
def test_normal_family_within_derived_bounds(ctx, guards, monkeypatch, cus, name):
    k = P.normal_case(name)
    n, h, w, cout = k.shape
    pair = P.NORMAL_PAIR
    dev = Dev(ctx, guards, k)
    worst = {}

    def keep(family, **ratios):
        for q, v in ratios.items():
            worst[f"{family}:{q}"] = max(worst.get(f"{family}:{q}", 0.0), v)

    for form in ("direct", "gemm"):
        env = use(monkeypatch, P.FORM_ENV[form])
        if form == "direct" and not P.direct_eligible(cout):
            continue
        for variant in ("stats", "bias"):
            y_ref = P.ref_fwd(k, pair, variant == "bias")
            y_b = P.fwd_bound(k, pair, form == "direct", variant == "bias")
            y, fold = fwd(ctx, dev, env, pair, variant)
            keep(form, y=ratio(y, y_ref, y_b))
            if fold is not None:
                s_b, q_b = P.stats_bounds(y_ref, y_b)
                keep(form, sum=ratio(fold[0], y_ref.sum(axis=(0, 1, 2)), s_b + 1e-300), sumsq=ratio(fold[1], (y_ref * y_ref).sum(axis=(0, 1, 2)), q_b + 1e-300))
    use(monkeypatch, {})
    plan = P.wgrad_plan(P.m_of(name), cout, cus)
    for gview, with_dbias in P.WGRAD_FORMS:
        dw_ref, db_ref = P.ref_bwd(k, pair, gview)
        dw_b, db_b = P.bwd_bounds(k, pair, gview)
        dw, db = bwd_weight(ctx, dev, pair, gview, with_dbias, plan)
        keep("wgrad", dW=ratio(dw, dw_ref, dw_b + 1e-300))
        if db is not None:
            keep("wgrad", dbias=ratio(db, db_ref, db_b + 1e-300))
    ctx.sync()
    guards.check()
    report("stem-normal", name, **worst)


# ----------------------------------------------------------------------------------------------------- fallback, contracts
@pytest.mark.parametrize("name", ["fallback-68", "fallback-100"])
def test_wide_stems_fall_back_to_the_implicit_gemm(ctx, guards, monkeypatch, name):
    """cout > 64 under the default switches: the rowA kernel, not the direct one, in the timing registry"""
    k = P.lattice_case(name)
    n, h, w, cout = k.shape
    use(monkeypatch, {})
    dev = Dev(ctx, guards, k)
    y = dev.fresh("y")
    kernels = run(ctx, lambda: ctx.call("ssdseg_stem_conv_fwd", dev.buf("x"), dev.buf("w"), None, y, n, h, w, 3, cout, 0.25, -0.5, None),
                  r"^gemm_rowA_kernel<\d, 0, 2, 0, 0, 0>$")
    assert not P.reaches(kernels, "stem_fwd_direct_kernel") and not P.direct_eligible(cout), kernels
    assert ratio(y.download().reshape(n, *k.geo[:2], cout), P.ref_fwd(k, P.PAIRS[1]), 0.0) == 0.0


def test_stem_argument_contracts(ctx, guards, monkeypatch):
    """rejected before any launch: nothing in the timing registry, the outputs still poison"""
    from ssdseglib import _hip as H
    use(monkeypatch, {})
    k = P.lattice_case("inst-2")
    n, h, w, cout = k.shape
    dev = Dev(ctx, guards, k)
    x, wgt, b, y, table, dw, db = (dev.buf(nm) for nm in ("x", "w", "b", "y", "stats", "dW", "dbias"))
    g = dev.buf("g")

    def refused(entry, *args):
        kernels = launched(ctx, lambda: rejected(ctx, entry, *args))
        assert kernels == {}, (entry, kernels)

    def fwd_args(x=x, wgt=wgt, bias=None, y=y, dims=(n, h, w), cin=3, cout=cout, stats=table):
        return (x, wgt, bias, y) + tuple(dims) + (cin, cout, 0.25, -0.5, stats)

    for bad in (dict(cin=4), dict(cin=1), dict(cout=0), dict(cout=6), dict(bias=b), dict(x=None), dict(wgt=None), dict(y=None),
                dict(dims=(0, h, w)), dict(dims=(n, 0, w)), dict(dims=(n, h, 0))):
        refused("ssdseg_stem_conv_fwd", *fwd_args(**bad))

    def bwd_args(x=x, gv=None, dw=dw, db=None, dims=(n, h, w), cin=3, cout=cout):
        return (x, gv if gv is not None else H.gview(g), dw, db) + tuple(dims) + (cin, cout, 0.25, -0.5)

    parts = [dev.buf(nm) for nm in ("yraw", "gscale", "gshift", "k1", "k0")]
    no_y = H.gview(g, None, *parts[1:], act=O.ACT_RELU6)
    full = H.gview(g, *parts, act=O.ACT_RELU6)
    for bad in (dict(gv=no_y), dict(gv=full, db=db), dict(dw=None), dict(x=None), dict(gv=H.gview(None)), dict(cin=4), dict(cout=0), dict(cout=6),
                dict(dims=(0, h, w)), dict(dims=(n, 0, w)), dict(dims=(n, h, 0))):
        args = bwd_args(**bad)
        if bad.get("dw", dw) is None:
            args = args[:2] + (None,) + args[3:]
        refused("ssdseg_stem_conv_bwd_weight", *args)
    # a NULL ctx is argument 1 (no ctx: the call goes to the library directly)
    for entry, args in (("ssdseg_stem_conv_fwd", fwd_args()), ("ssdseg_stem_conv_bwd_weight", bwd_args())):
        conv = [C.c_void_p(a.ptr) if isinstance(a, H.DeviceBuffer) else (C.byref(a) if isinstance(a, H.GViewStruct) else a) for a in args]
        kernels = launched(ctx, lambda: conv.append(getattr(ctx.lib, entry)(None, *conv)))
        assert conv[-1] == -1001 and kernels == {}, (entry, conv[-1], kernels)
    out = C.c_int()
    for dims, arg in (((0, h, w, cout), 1), ((n, 0, w, cout), 1), ((n, h, 0, cout), 1), ((n, h, w, 0), 4), ((n, h, w, 6), 4)):
        assert ctx.lib.ssdseg_stem_conv_parts(*dims, C.byref(out)) == -1000 - arg, dims
    assert ctx.lib.ssdseg_stem_conv_parts(n, h, w, cout, None) == -1005
    ctx.sync()
    for o in (y, table, dw, db):
        assert untouched(o) == o.size


# ------------------------------------------------------------------------------------------------------------ the max-pool
def pool_dev(guards, k, view):
    from ssdseglib import _hip as H
    xb = guards.inp(k.x, name="pool x")
    if view == "plain":
        return H.view(xb)
    return H.view(xb, guards.inp(k.scale, name="pool scale"), guards.inp(k.shift, name="pool shift"), view)


def pool_check(ctx, guards, monkeypatch, k, view):
    """forward == oracle; default backward == scan backward bit for bit == oracle; dx fully written; sum dx == sum g per channel; the
    repeated image gives the same bits"""
    n, h, w, c = k.shape
    ho, wo = k.geo[:2]
    v = pool_dev(guards, k, view)
    a = P.pool_in(k, view)
    out = guards.out((n, ho, wo, c), name="pool out")
    run(ctx, lambda: ctx.call("ssdseg_maxpool3x3s2_fwd", v, out, n, h, w, c), "^maxpool_fwd_kernel$")
    y = out.download()
    assert poisoned(y) == 0 and ratio(y, O.maxpool3x3s2_fwd(a), 0.0) == 0.0, "forward"
    gout = guards.inp(k.g, name="pool g")
    dx_ref = O.maxpool3x3s2_bwd(a, k.g.astype(np.float64))
    got = {}
    for mode, patterns in ((None, ("^maxpool_argmax_kernel$", "^maxpool_bwd_codes_kernel$")), ("scan", ("^maxpool_bwd_kernel$",))):
        use(monkeypatch, {"SSDSEG_MAXPOOL_BWD": mode} if mode else {})
        dx = guards.out((n, h, w, c), name=f"pool dx {mode}")
        run(ctx, lambda: ctx.call("ssdseg_maxpool3x3s2_bwd", v, gout, dx, n, h, w, c), *patterns)
        assert untouched(dx) == 0, "an element of dx was not written"
        got[mode] = dx.download()
        assert ratio(got[mode], dx_ref, 0.0) == 0.0, ("backward", mode)
        assert np.array_equal(got[mode].astype(np.float64).sum(axis=(0, 1, 2)), k.g.astype(np.float64).sum(axis=(0, 1, 2))), "sum dx != sum g"
        assert same_bits(got[mode][0], got[mode][-1]), "the repeated image differs"
    assert same_bits(got[None], got["scan"]), "the two backward forms differ in bits"
    assert same_bits(y[0], y[-1])
    ctx.sync()
    guards.check()
    return a, got[None]


@pytest.mark.parametrize("shape", P.POOL_SHAPES, ids=lambda s: "x".join(str(d) for d in s))
def test_pool_is_exact_under_every_view(ctx, guards, monkeypatch, shape):
    k = P.pool_case(shape)
    for view in P.POOL_VIEWS:
        pool_check(ctx, guards, monkeypatch, k, view)


def test_pool_ties_go_to_the_first_valid_cell(ctx, guards, monkeypatch):
    """every pre-activation negative under ReLU: every window is a tie among all its valid cells, and the whole gradient of a window
    lands on the first of them in the row-major scan -- at a top or left border that is not tap 0"""
    k = P.pool_case(P.POOL_SPECIAL["all-negative"], "all-negative")
    a, dx = pool_check(ctx, guards, monkeypatch, k, O.ACT_RELU)
    assert not a.any()
    first_valid = np.isfinite(P.pool_windows(a)).argmax(axis=0)
    assert (first_valid != 0).any()
    assert np.array_equal(dx, P.pool_bwd_by(a, k.g.astype(np.float64), P.one_hot(first_valid)))


def test_pool_signed_zeros(ctx, guards, monkeypatch):
    """-0.0 and +0.0 in one window: the forward value is compared as a number, the gradient goes to the first of them"""
    k = P.pool_case(P.POOL_SPECIAL["signed-zeros"], "signed-zeros")
    pool_check(ctx, guards, monkeypatch, k, "plain")


def test_pool_argument_contracts(ctx, guards, monkeypatch):
    from ssdseglib import _hip as H
    use(monkeypatch, {})
    k = P.pool_case((2, 3, 4, 4))
    n, h, w, c = k.shape
    xb, sc, sh, g = (guards.inp(a) for a in (k.x, k.scale, k.shift, k.g))
    out, dx = guards.out((n,) + k.geo[:2] + (c,)), guards.out(k.shape)
    v = H.view(xb)

    def refused(entry, *args):
        kernels = launched(ctx, lambda: rejected(ctx, entry, *args))
        assert kernels == {}, (entry, kernels)

    for view in (H.view(xb, sc, None, O.ACT_RELU), H.view(xb, None, sh, O.ACT_RELU), H.view(None), None):
        refused("ssdseg_maxpool3x3s2_fwd", view, out, n, h, w, c)
        refused("ssdseg_maxpool3x3s2_bwd", view, g, dx, n, h, w, c)
    refused("ssdseg_maxpool3x3s2_fwd", v, None, n, h, w, c)
    refused("ssdseg_maxpool3x3s2_bwd", v, None, dx, n, h, w, c)
    refused("ssdseg_maxpool3x3s2_bwd", v, g, None, n, h, w, c)
    for dims in ((0, h, w, c), (n, 0, w, c), (n, h, 0, c), (n, h, w, 0), (n, h, w, 6)):
        refused("ssdseg_maxpool3x3s2_fwd", v, out, *dims)
        refused("ssdseg_maxpool3x3s2_bwd", v, g, dx, *dims)
    ctx.sync()
    assert untouched(out) == out.size and untouched(dx) == dx.size


# --------------------------------------------------------------------------------------------------------------- coverage
def test_the_suite_reaches_every_direct_instantiation():
    """every stem_fwd_direct_kernel<Q>, both forms of the implicit GEMM's occupancy, and the weight gradient at wn = 1, 2, 3 are among
    the launches the timing registry recorded, when every lattice case ran in this process"""
    if not RAN >= set(P.CASES):
        pytest.skip("not every lattice case ran in this process: the recorded launches are not the suite's")
    want = [r"^stem_fwd_direct_kernel<%d>$" % q for q in range(1, 17)] + [r"^gemm_rowA_kernel<%d, 0, 2, 0, 0, 0>$" % wn for wn in (1, 3, 5)] + \
        [r"^gemm_rowA_kernel<1, 0, 2, 0, 0, 1>$"] + [r"^gemm_wgrad_kernel<1, 4, %d> \[conv3x3 tap\]$" % wn for wn in (1, 2, 3)] + \
        ["^colsum_kernel$", "^maxpool_fwd_kernel$", "^maxpool_argmax_kernel$", "^maxpool_bwd_codes_kernel$", "^maxpool_bwd_kernel$"]
    assert [p for p in want if not P.reaches(RECORDED, p)] == []
