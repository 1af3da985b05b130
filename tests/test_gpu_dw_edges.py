"""GPU parity of the depthwise 3x3 conv kernels at their edges (through the C-ABI) vs float64.

ssdseg_dwconv_parts / _fwd / _bwd / _bwd_bn (csrc/dwconv.hip, csrc/dwconv_march.h, csrc/dwconv_lds.h) on the cases of
tests/_dw_cases.py: row chunks of 1, 2, 3 and 8 rows, 5 + 4, 7 + 6, 5 + 5 + 5 + 2 and 7 x 6 + 1 rows at both strides, a halving that stops
midway, the one-chunk march over more than 8 rows, widths 1 .. 9, a wasted strip slot and two strip groups, the four stride-2 pad
pairs at one and at three output columns, 4 .. 1284 channels, five dilations under the march and under the gather kernels, and the
grid-stride second trip of the register-window, gather and LDS kernels -- each under every kernel family that takes it
(SSDSEG_DW_FWD / _BWD / _ATROUS / _FWD_DEPTH, read per call), each form of the two views, with and without dx, statistics and
accumulation.  tests/test_cpu_dw_cases.py vets the reference, the cases and the mirror of the launch geometry.  Every buffer is
guarded (tests/_guard.py); every launch is read from the timing registry.

Bounds.  U = 2^-24, gamma(L) = L U / (1 - L U).

  lattice family   0 for y, dx, dW, every row fold of the statistics table and the fused dgamma / dbeta: the inputs are small multiples
                   of powers of two and every reduction stays below 2^24 units of its lattice (_dw_cases.budget), so float32
                   arithmetic is exact in any order, fused or not, and every family must give the same numbers: each result is
                   also compared bit for bit with the first family's, after x + 0 on both.  (The sign of a zero is not part of
                   the claim: a product 0 * -w is -0 where another family adds it to +0.)
  k1, k0           U |k| + 2^-50 of the absolute terms of their formulas: the finalize kernel works in float64 from the exact sums
                   and rounds once.
  normal family    a = act(s x + t) is one fused multiply-add: |da| <= U (|s x| + |t|); the clamp does not amplify it.
                   y: nine multiply-adds over the taps and the view's rounding: (gamma(9 + 1) + U) sum A |w|, A = |s x| + |t| >= |a|.
                   dy = s m g + (k1 y + k0) is two roundings of its absolute terms D = |s g| + |k1 y| + |k0| (identity: D = |g|, exact);
                   the mask is safe: |z| U < 1e-6 << the 1e-4 band.  dx: gamma(9 + 1) sum D |w| + 2 U sum D |w|; with accumulate one
                   more rounding of the total.
                   dW: a chain of L = trips x outputs-per-trip + strips-per-block float32 additions (the mirror's counts), then
                   float64 and one rounding: (gamma(L + 2) + 3 U) sum A D + U |dW|.
                   statistics: gamma(L + 1) sum |y| + sum of the y bounds; gamma(L + 2) sum y^2 + sum (2 |y| b + b^2).
                   fused sums: gamma(L + 1) sum |m dx| + sum of the dx bounds, the same with |xhat| and 2 U for xhat's two roundings,
                   + one rounding of the result; the unfused path with the chain of ssdseg_bn_bwd_reduce.

Run with -s for the largest error / bound ratio of every case (DESIGN.md records them).
"""
import os

import numpy as np
import pytest

import _dw_cases as D
from oracle import np_ops as O
from _guard import BODY_WORD, guards  # noqa: F401  (fixture)
from _edge_helpers import launched, ratio, rejected, reporter, same_bits, untouched

pytestmark = pytest.mark.gpu

F32 = np.float32
report = reporter("dw-edges")


@pytest.fixture(autouse=True)
def march_switches_unset():
    """SSDSEG_MARCH_WAVES / _CB / _MAXT are read once per process: the mirror describes the geometry without them"""
    present = [v for v in D.MARCH_ENV if v in os.environ]
    assert not present, f"{present} set: the launch geometry of the marching kernels is not the one these tests describe"


def use(monkeypatch, setting):
    for v in D.DW_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, value in D.SETTINGS[setting].items():
        monkeypatch.setenv(v, value)
    return D.SETTINGS[setting]


def poisoned(a):
    return int((np.ascontiguousarray(a).view(np.uint32) == np.uint32(BODY_WORD)).sum())


class Dev:
    """the inputs of one case on the device, guarded, and the outputs its calls share"""

    def __init__(self, guards, k):
        n, h, w, c, s, d = k.shape
        self.k = k
        for f in ("x", "w", "g", "yraw", "scale", "shift", "gscale", "gshift", "k1", "k0", "mean", "invstd"):
            setattr(self, f, guards.inp(getattr(k, f), name=f))
        self.y = guards.out((n, k.ho, k.wo, c), name="y")
        self.dx = guards.out((n, h, w, c), name="dx")
        self.dw = guards.out((3, 3, c), name="dW")
        self.bn = [guards.out((c,), name=f) for f in ("dgamma", "dbeta", "k1out", "k0out")]

    def view(self, view):
        from ssdseglib import _hip as H
        return H.view(self.x) if view == "plain" else H.view(self.x, self.scale, self.shift, view)

    def gview(self, gview):
        from ssdseglib import _hip as H
        if gview == "identity":
            return H.gview(self.g)
        return H.gview(self.g, self.yraw, self.gscale, self.gshift, self.k1, self.k0, act=gview)


def conv_launches(kernels, plan, extra):
    """one launch of the instantiation the mirror names -- template flags included (BNFUSE, WFULL, ACC, DIL, the pads, D2) -- and
    exactly the reductions in `extra`"""
    assert kernels == dict(extra, **{plan["symbol"]: 1}), (kernels, plan["symbol"], extra)


def fwd(ctx, guards, dev, view, stats, env, table):
    n, h, w, c, s, d = dev.k.shape
    guards.repoison(dev.y)
    guards.repoison(table)
    plan = D.fwd_plan_env(n, h, w, c, s, d, env)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_dwconv_fwd", dev.view(view), dev.w, dev.y, n, h, w, c, s, d, table if stats else None))
    conv_launches(kernels, plan, {})
    y = dev.y.download()
    assert poisoned(y) == 0
    if not stats:
        assert untouched(table) == table.size
        return y, None, plan
    return y, table.download(), plan


def table_rows(t, plan):
    """the claims about the statistics table, row by row; -> its float64 fold (2, c)"""
    assert poisoned(t) == 0 and np.isfinite(t).all(), "a row of the statistics table was not written"
    assert not t[plan["rows"]:].any(), "rows beyond the launch's own count are not zero"
    assert not t[plan["live"]:plan["rows"]].any(), "a surplus block wrote a non-zero row"
    return t.astype(np.float64).sum(axis=0)


def bwd(ctx, guards, dev, view, gview, has_dx, accumulate, env):
    n, h, w, c, s, d = dev.k.shape
    guards.repoison(dev.dw)
    guards.repoison(dev.dx)
    if accumulate and has_dx:
        dev.dx.upload(dev.k.base)
    plan = D.bwd_plan(n, h, w, c, s, d, env, has_dx=has_dx, accumulate=bool(accumulate))
    kernels = launched(ctx, lambda: ctx.call("ssdseg_dwconv_bwd", dev.view(view), dev.w, dev.gview(gview), dev.dx if has_dx else None, dev.dw,
                                             n, h, w, c, s, d, accumulate))
    conv_launches(kernels, plan, {"colsum_kernel": 1})
    dw = dev.dw.download()
    assert poisoned(dw) == 0
    if not has_dx:
        assert untouched(dev.dx) == dev.dx.size
        return None, dw, plan
    dx = dev.dx.download()
    assert poisoned(dx) == 0
    return dx, dw, plan


def bwd_bn(ctx, guards, dev, view, gview, accumulate, env):
    n, h, w, c, s, d = dev.k.shape
    for b in [dev.dw, dev.dx] + dev.bn:
        guards.repoison(b)
    if accumulate:
        dev.dx.upload(dev.k.base)
    plan = D.bwd_plan(n, h, w, c, s, d, env, has_dx=True, accumulate=bool(accumulate), has_bn=True)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_dwconv_bwd_bn", dev.view(view), dev.w, dev.gview(gview), dev.dx, dev.dw, n, h, w, c, s, d,
                                             accumulate, dev.mean, dev.invstd, *dev.bn))
    extra = {"colsum_kernel": 1, "bn_bwd_finalize_kernel": 1}
    if not plan["fuse"]:
        extra["bn_bwd_partial_kernel"] = 1
    conv_launches(kernels, plan, extra)
    outs = [b.download() for b in [dev.dx, dev.dw] + dev.bn]
    assert all(poisoned(o) == 0 for o in outs)
    return outs, plan


# ------------------------------------------------------------------------------------------------------- lattice: bound 0
@pytest.mark.parametrize("name", list(D.CASES))
def test_lattice_is_exact_in_every_family(ctx, guards, monkeypatch, name):
    """every form of every entry point, under every family that takes the case: y, dx, dW, the row fold of the statistics and the
    fused dgamma / dbeta equal the float64 reference (bound 0), so the families equal each other; k1 / k0 within their rounding"""
    k = D.lattice_case(name)
    n, h, w, c, s, d = k.shape
    fwd_forms, bwd_forms, bn_forms = D.forms_of(name)
    dev = Dev(guards, k)
    nparts = ctx.parts("ssdseg_dwconv_parts", n, h, w, c, s, d)
    assert nparts == D.dw_fwd_table_rows(n, h, w, c, s, d)
    table = guards.out((nparts, 2, c), name="stats")
    refs, first, kratio, families = {}, {}, 0.0, set()

    def ref(key, make):
        if key not in refs:
            refs[key] = make()
        return refs[key]

    def same_as_first(key, setting, *arrays):
        """family against family, directly: the bits of the first setting's results, the sign of a zero normalised (x + 0)"""
        kept = first.setdefault(key, (setting, [a + F32(0) for a in arrays]))
        for got, want in zip(arrays, kept[1]):
            assert same_bits(got + F32(0), want), (key, setting, "differs in bits from", kept[0])

    for setting in D.settings_of(name):
        env = use(monkeypatch, setting)
        for view, stats in fwd_forms:
            y_ref, s_ref, q_ref = ref(("fwd", view), lambda: D.ref_fwd(k, view))
            y, t, plan = fwd(ctx, guards, dev, view, stats, env, table)
            families.add(plan["kernel"])
            assert ratio(y, y_ref, 0.0) == 0.0, (setting, "fwd", D.form_name((view, stats)))
            same_as_first(("fwd", view, stats), setting, y)
            if stats:
                fold = table_rows(t, plan)
                assert ratio(fold[0], s_ref, 0.0) == 0.0 and ratio(fold[1], q_ref, 0.0) == 0.0, (setting, "stats", D.form_name((view,)))
        for view, gview, has_dx, accumulate in bwd_forms:
            dx_ref, dw_ref = ref(("bwd", view, gview, accumulate and has_dx), lambda: D.ref_bwd(k, view, gview, accumulate and has_dx))
            dx, dw, plan = bwd(ctx, guards, dev, view, gview, has_dx, accumulate, env)
            families.add(plan["kernel"])
            what = (setting, "bwd", D.form_name((view, gview, has_dx, accumulate)))
            assert ratio(dw, dw_ref, 0.0) == 0.0, what
            same_as_first(("bwd", view, gview, has_dx, accumulate, "dW"), setting, dw)
            if has_dx:
                assert ratio(dx, dx_ref, 0.0) == 0.0, what
                same_as_first(("bwd", view, gview, accumulate, "dx"), setting, dx)
            if view == O.ACT_ZERO:
                assert not dw.any(), what
        for view, gview, accumulate in bn_forms:
            r = ref(("bn", view, gview, accumulate), lambda: D.ref_bn(k, view, gview, accumulate))
            (dx, dw, dgamma, dbeta, k1, k0), plan = bwd_bn(ctx, guards, dev, view, gview, accumulate, env)
            what = (setting, "bwd_bn", D.form_name((view, gview, accumulate)), "fused" if plan["fuse"] else "unfused")
            for got, want in zip((dx, dw, dgamma, dbeta), r[:4]):
                assert ratio(got, want, 0.0) == 0.0, what
            same_as_first(("bn", view, gview, accumulate), setting, dx, dw, dgamma, dbeta)
            kratio = max(kratio, ratio(k1, r[4], r[6][0] + 1e-300), ratio(k0, r[5], r[6][1] + 1e-300))
    assert families
    report("dwconv", name, k1k0=kratio)


TWINS = ["rows9", "rows17-s2", "strips-wasted", "strips-wasted-s2", "chan260", "dil2-5x7", "pads-6x5-s2"]


@pytest.mark.parametrize("name", TWINS)
def test_an_image_does_not_depend_on_its_batch_position(ctx, guards, monkeypatch, name):
    k = D.twin_case(name)
    n, h, w, c, s, d = k.shape
    assert n >= 2
    dev = Dev(guards, k)
    table = guards.out((ctx.parts("ssdseg_dwconv_parts", n, h, w, c, s, d), 2, c), name="stats")
    for setting in D.settings_of(name):
        env = use(monkeypatch, setting)
        y, _, _ = fwd(ctx, guards, dev, O.ACT_RELU6, True, env, table)
        assert np.array_equal(y[0], y[-1]), setting
        for accumulate in (0, 1):
            dx, _, _ = bwd(ctx, guards, dev, O.ACT_RELU6, O.ACT_RELU6, True, accumulate, env)
            assert np.array_equal(dx[0], dx[-1]), (setting, accumulate)


FAMILY_CASES = ["rows13", "rows9-s2", "cols5", "chan144", "dil3-7x5"]


@pytest.mark.parametrize("name", FAMILY_CASES)
def test_lattice_under_the_suite_wide_kernel_families(ctx, guards, kernel_family, name):
    """the families of tests/conftest.py as they are: the forward with statistics, one backward and the fused form"""
    k = D.lattice_case(name)
    n, h, w, c, s, d = k.shape
    env = {v: os.environ[v] for v in D.DW_VARS if v in os.environ}
    dev = Dev(guards, k)
    table = guards.out((ctx.parts("ssdseg_dwconv_parts", n, h, w, c, s, d), 2, c), name="stats")
    y_ref, s_ref, q_ref = D.ref_fwd(k, O.ACT_RELU6)
    y, t, plan = fwd(ctx, guards, dev, O.ACT_RELU6, True, env, table)
    fold = table_rows(t, plan)
    assert ratio(y, y_ref, 0.0) == 0.0 and ratio(fold[0], s_ref, 0.0) == 0.0 and ratio(fold[1], q_ref, 0.0) == 0.0
    dx_ref, dw_ref = D.ref_bwd(k, O.ACT_RELU6, O.ACT_RELU6, 1)
    dx, dw, _ = bwd(ctx, guards, dev, O.ACT_RELU6, O.ACT_RELU6, True, 1, env)
    assert ratio(dx, dx_ref, 0.0) == 0.0 and ratio(dw, dw_ref, 0.0) == 0.0
    r = D.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6, 1)
    (dx, dw, dgamma, dbeta, k1, k0), _ = bwd_bn(ctx, guards, dev, O.ACT_RELU6, O.ACT_RELU6, 1, env)
    for got, want in zip((dx, dw, dgamma, dbeta), r[:4]):
        assert ratio(got, want, 0.0) == 0.0
    report("dwconv-family", f"{name}-{kernel_family}", k1=ratio(k1, r[4], r[6][0] + 1e-300), k0=ratio(k0, r[5], r[6][1] + 1e-300))


# ------------------------------------------------------------------------------------------------ normal: derived bounds
@pytest.mark.parametrize("name", D.NORMAL_CASES)
def test_normal_family_within_derived_bounds(ctx, guards, monkeypatch, name):
    k = D.normal_case(name)
    n, h, w, c, s, d = k.shape
    dev = Dev(guards, k)
    table = guards.out((ctx.parts("ssdseg_dwconv_parts", n, h, w, c, s, d), 2, c), name="stats")
    worst = {}

    def keep(plan, **ratios):
        for q, v in ratios.items():
            key = f"{plan['family']}:{q}"
            worst[key] = max(worst.get(key, 0.0), v)

    for setting in D.settings_of(name) + ("march",):
        env = use(monkeypatch, setting)
        for view, gview, accumulate in ((O.ACT_RELU6, O.ACT_RELU6, 0), (O.ACT_RELU6, O.ACT_RELU6, 1), ("plain", "identity", 0),
                                        (O.ACT_NONE, O.ACT_RELU, 1)):
            fplan = D.fwd_plan_env(n, h, w, c, s, d, env)
            bplan = D.bwd_plan(n, h, w, c, s, d, env, True, bool(accumulate), view != "plain")
            b = D.normal_bounds(k, view, gview, accumulate, fplan, bplan)
            y_ref, s_ref, q_ref = D.ref_fwd(k, view)
            y, t, plan = fwd(ctx, guards, dev, view, True, env, table)
            fold = table_rows(t, plan)
            keep(fplan, y=ratio(y, y_ref, b["y"]), sum=ratio(fold[0], s_ref, b["sum"]), sumsq=ratio(fold[1], q_ref, b["sumsq"]))
            dx_ref, dw_ref = D.ref_bwd(k, view, gview, accumulate)
            if view == "plain":
                dx, dw, _ = bwd(ctx, guards, dev, view, gview, True, accumulate, env)
                keep(bplan, dx=ratio(dx, dx_ref, b["dx"]), dW=ratio(dw, dw_ref, b["dW"]))
                continue
            r = D.ref_bn(k, view, gview, accumulate)
            (dx, dw, dgamma, dbeta, k1, k0), _ = bwd_bn(ctx, guards, dev, view, gview, accumulate, env)
            keep(bplan, dx=ratio(dx, dx_ref, b["dx"]), dW=ratio(dw, dw_ref, b["dW"]), dgamma=ratio(dgamma, r[2], b["dgamma"]),
                 dbeta=ratio(dbeta, r[3], b["dbeta"]))
    report("dwconv-normal", name, **worst)


# ----------------------------------------------------------------------------------------------------- argument contracts
def test_argument_contracts(ctx, guards, monkeypatch):
    """every bad call is rejected before any launch: nothing in the timing registry, the outputs still poison"""
    from ssdseglib import _hip as H
    use(monkeypatch, "default")
    k = D.lattice_case("cols5")
    n, h, w, c, s, d = k.shape
    dev = Dev(guards, k)
    table = guards.out((8, 2, c), name="stats")
    outs = [dev.y, dev.dx, dev.dw, table] + dev.bn
    good = dict(n=n, h=h, w=w, c=c, s=1, d=1)
    bad_dims = [dict(c=6), dict(c=0), dict(s=0), dict(s=3), dict(d=0), dict(d=-1), dict(s=2, d=2), dict(n=0), dict(n=-1), dict(h=0),
                dict(h=-3), dict(w=0), dict(w=-1)]
    vin, gv = dev.view(O.ACT_RELU6), dev.gview(O.ACT_RELU6)
    half_view = H.view(dev.x, dev.scale, None, O.ACT_RELU6)
    half_view2 = H.view(dev.x, None, dev.shift, O.ACT_RELU6)

    def half_gview(missing):
        parts = dict(y=dev.yraw, scale=dev.gscale, shift=dev.gshift, k1=dev.k1, k0=dev.k0)
        parts[missing] = None
        return H.gview(dev.g, parts["y"], parts["scale"], parts["shift"], parts["k1"], parts["k0"], act=O.ACT_RELU6)

    calls = []
    for bad in bad_dims:
        q = dict(good, **bad)
        dims = (q["n"], q["h"], q["w"], q["c"], q["s"], q["d"])
        calls.append(("ssdseg_dwconv_fwd", (vin, dev.w, dev.y) + dims + (table,)))
        calls.append(("ssdseg_dwconv_bwd", (vin, dev.w, gv, dev.dx, dev.dw) + dims + (0,)))
        calls.append(("ssdseg_dwconv_bwd_bn", (vin, dev.w, gv, dev.dx, dev.dw) + dims + (0, dev.mean, dev.invstd) + tuple(dev.bn)))
        with pytest.raises(H.SsdsegError, match="ssdseg_dwconv_parts: invalid argument"):
            ctx.parts("ssdseg_dwconv_parts", *dims)
    dims = (n, h, w, c, 1, 1)
    for v in (H.view(None), half_view, half_view2):
        calls.append(("ssdseg_dwconv_fwd", (v, dev.w, dev.y) + dims + (table,)))
        calls.append(("ssdseg_dwconv_bwd", (v, dev.w, gv, dev.dx, dev.dw) + dims + (0,)))
        calls.append(("ssdseg_dwconv_bwd_bn", (v, dev.w, gv, dev.dx, dev.dw) + dims + (0, dev.mean, dev.invstd) + tuple(dev.bn)))
    calls.append(("ssdseg_dwconv_fwd", (None, dev.w, dev.y) + dims + (table,)))
    calls.append(("ssdseg_dwconv_fwd", (vin, None, dev.y) + dims + (table,)))
    calls.append(("ssdseg_dwconv_fwd", (vin, dev.w, None) + dims + (table,)))
    for entry, tail in (("ssdseg_dwconv_bwd", (0,)), ("ssdseg_dwconv_bwd_bn", (0, dev.mean, dev.invstd) + tuple(dev.bn))):
        calls.append((entry, (None, dev.w, gv, dev.dx, dev.dw) + dims + tail))
        calls.append((entry, (vin, None, gv, dev.dx, dev.dw) + dims + tail))
        calls.append((entry, (vin, dev.w, None, dev.dx, dev.dw) + dims + tail))
        calls.append((entry, (vin, dev.w, H.gview(None), dev.dx, dev.dw) + dims + tail))
        calls.append((entry, (vin, dev.w, gv, dev.dx, None) + dims + tail))
        for missing in ("y", "shift", "k1", "k0"):
            calls.append((entry, (vin, dev.w, half_gview(missing), dev.dx, dev.dw) + dims + tail))
    # the fused form: an affine input view, dx, the statistics and the two coefficient outputs are required (dgamma / dbeta are not)
    bn = ("ssdseg_dwconv_bwd_bn", (vin, dev.w, gv, dev.dx, dev.dw) + dims)
    calls.append((bn[0], (dev.view("plain"),) + bn[1][1:] + (0, dev.mean, dev.invstd) + tuple(dev.bn)))
    calls.append((bn[0], (vin, dev.w, gv, None, dev.dw) + dims + (0, dev.mean, dev.invstd) + tuple(dev.bn)))
    calls.append((bn[0], bn[1] + (0, None, dev.invstd) + tuple(dev.bn)))
    calls.append((bn[0], bn[1] + (0, dev.mean, None) + tuple(dev.bn)))
    calls.append((bn[0], bn[1] + (0, dev.mean, dev.invstd, dev.bn[0], dev.bn[1], None, dev.bn[3])))
    calls.append((bn[0], bn[1] + (0, dev.mean, dev.invstd, dev.bn[0], dev.bn[1], dev.bn[2], None)))
    calls.append((bn[0], (vin, dev.w, gv, dev.dx, dev.dw, 46341, 46341, 1, 4, 1, 1, 0, dev.mean, dev.invstd) + tuple(dev.bn)))   # n h w > 2^31 - 1
    for entry, args in calls:
        kernels = launched(ctx, lambda: rejected(ctx, entry, *args))
        assert kernels == {}, (entry, kernels)
    for o in outs:
        assert untouched(o) == o.size
    # and the good call still runs
    (dx, dw, dgamma, dbeta, k1, k0), _ = bwd_bn(ctx, guards, dev, O.ACT_RELU6, O.ACT_RELU6, 0, {})
    r = D.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6, 0)
    assert ratio(dx, r[0], 0.0) == 0.0 and ratio(dgamma, r[2], 0.0) == 0.0
