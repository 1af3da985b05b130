"""GPU parity of the pointwise (1x1) conv GEMMs at their edges (through the C-ABI) vs float64.

ssdseg_pwconv_parts / _fwd_wt / _bwd_data / _bwd_weight / _bwd / _bwd_bn (csrc/gemm.hip, csrc/gemm_wres.h, csrc/pw_tile.h,
csrc/pw_wgrad.hip, csrc/pw_wgrad.h) on the cases of tests/_pw_cases.py: 1 .. 257 rows around the 32-row wave tile, the 128-row block
tile and the 256-row eight-wave tile; reductions around one, two and three 32-deep steps; the last reduction that fits the resident
kernel's LDS and the first that does not; ragged column tiles; the eight-wave tile GEMM at every width and its 4 x 2 wave grid;
514 row tiles (the last with one row) at every rowA width, epilogue and occupancy form; grid-stride trips; the fused dx + dW
kernels at NT = 1 .. 6 and with waves that walk a second tile; every tile shape of the row-naming weight gradient at its step and
split edges; row pitches on every operand; unaligned outputs; the transposed weight copy; rejected calls -- each under the switch
settings that change its kernel (set per call with monkeypatch), each form of the two views.  tests/test_cpu_pw_cases.py vets the
reference, the cases and the mirror.  Every buffer is guarded (tests/_guard.py); every launch is read from the timing registry and
must be exactly what the mirror of the host rules names.

Bounds.  U = 2^-24, gamma(L) = L U / (1 - L U).

  lattice family   0 for y, dx in its four forms, dW, the row fold of the statistics table and the fused dgamma / dbeta: the inputs
                   are small multiples of powers of two and every reduction stays below 2^24 units of its lattice
                   (_pw_cases.budget); the MFMA's fp32 products are exact, so float32 arithmetic is exact in any order and every
                   kernel must give the same numbers: each result is also compared bit for bit with the first setting's, after
                   x + 0 on both (the sign of a zero is not part of the claim).  A stored and a recomputed y are the same number
                   on the lattice, so ssdseg_pwconv_bwd carries the conv's own output in its gradient view and nothing is zeroed.
  k1, k0           U |k| + 2^-50 of the absolute terms of their formulas: the finalize kernel works in float64 from the exact sums
                   and rounds once.
  normal family    any-order bounds, so no mirror of the accumulation order is needed.  a = act(s x + t) is one fused multiply-add:
                   |da| <= U A, A = |s x| + |t| >= |a|; the clamp does not amplify it.
                   y: K exact products summed in some order, at most K roundings on any path, and the view's rounding:
                   (gamma(K + 1) + U) sum_k A_k |w_k|.
                   dy = s m g + (k1 y + k0): two roundings of its absolute terms D = |s g| + |k1 y| + |k0| (identity: D = |g|, dy
                   exact); the mask is safe: |z| U < 1e-6 << the 1e-4 band.
                   dx: (gamma(N + 1) + 2 U) sum_n D_n |w_n|, plus one rounding of the running total per residual / accumulate term.
                   dW: a float32 chain of at most M terms, then the float64 column sum and one rounding:
                   (gamma(M + 2) + 3 U) sum_m A D + U |dW|.
                   statistics: gamma(M + 1) sum |y| + sum of the y bounds; gamma(M + 2) sum y^2 + sum (2 |y| b + b^2).
                   fused sums: gamma(M + 1) sum |m dx| + sum of the dx bounds, the same with |xhat| and 2 U for xhat's two roundings,
                   + one rounding of the result.

Run with -s for the largest error / bound ratio of every case (DESIGN.md records them).
"""
import os

import numpy as np
import pytest

import _pw_cases as P
from oracle import np_ops as O
from _guard import BODY_WORD, guards  # noqa: F401  (fixture)
from _edge_helpers import launched, ratio, rejected, reporter, same_bits, untouched

pytestmark = pytest.mark.gpu

F32 = np.float32
report = reporter("pw-edges")
RECORDED = set()        # every kernel symbol the timing registry showed in this process
RAN = set()             # the cases whose lattice test ran in this process


@pytest.fixture(autouse=True)
def once_per_process_switches_unset():
    """SSDSEG_WRES_LDS_KB is read once per process: the mirror describes the resident kernel's fit without it"""
    present = [v for v in P.ONCE_ENV if v in os.environ]
    assert not present, f"{present} set: the resident kernels' LDS budget is not the one these tests describe"


def use(monkeypatch, setting):
    for v in P.PW_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, value in P.SETTINGS[setting].items():
        monkeypatch.setenv(v, value)
    return P.SETTINGS[setting]


def poisoned(a):
    return int((np.ascontiguousarray(a).view(np.uint32) == np.uint32(BODY_WORD)).sum())


class Dev:
    """the operands of one case on the device, guarded, at the case's row pitches; allocated when first used"""

    def __init__(self, ctx, guards, k):
        self.ctx, self.guards, self.k, self.ld = ctx, guards, k, k.ld
        self._bufs = {}

    def buf(self, name):
        if name not in self._bufs:
            k, ld, g = self.k, self.ld, self.guards
            m, kk, n = k.shape
            if name in ("x", "res"):
                b = g.inp(getattr(k, name), ld=ld["x"] if name == "x" else ld["r"], name=name)
            elif name in ("g", "yraw"):
                b = g.inp(getattr(k, name), ld=ld["y"], name=name)
            elif name.startswith("own:"):
                view = name[4:]
                b = g.inp(P.own_y(k, view if view == "plain" else int(view)), ld=ld["y"], name=name)
            elif name == "y":
                b = g.out((m, n), ld=ld["y"], name=name)
            elif name == "dx":
                b = g.out((m, kk), ld=ld["dx"], name=name)
            elif name == "dW":
                b = g.out((kk, n), name=name)
            elif name in ("dgamma", "dbeta", "k1out", "k0out"):
                b = g.out((kk,), name=name)
            elif name == "stats":
                b = g.out((self.ctx.parts("ssdseg_pwconv_parts", m, n), 2, n), name=name)
            else:
                b = g.inp(getattr(k, name), name=name)
            self._bufs[name] = b
        return self._bufs[name]

    def view(self, view):
        from ssdseglib import _hip as H
        return H.view(self.buf("x")) if view == "plain" else H.view(self.buf("x"), self.buf("scale"), self.buf("shift"), view)

    def gview(self, gview, own=None):
        from ssdseglib import _hip as H
        if gview == "identity":
            return H.gview(self.buf("g"))
        y = self.buf("yraw") if own is None else self.buf(f"own:{own}")
        return H.gview(self.buf("g"), y, self.buf("gscale"), self.buf("gshift"), self.buf("k1"), self.buf("k0"), act=gview)

    def fresh(self, *names):
        out = [self.guards.repoison(self.buf(nm)) for nm in names]
        return out if len(out) > 1 else out[0]


def run(ctx, fn, want):
    """the launches of fn(): exactly what the mirror names"""
    kernels = launched(ctx, fn)
    RECORDED.update(kernels)
    assert kernels == want, ("launched", kernels, "the mirror names", want)


def fwd(ctx, dev, view, stats, want, wt=None):
    m, kk, n = dev.k.shape
    y, table = dev.fresh("y", "stats")
    run(ctx, lambda: ctx.call("ssdseg_pwconv_fwd_wt", dev.view(view), dev.ld["x"], dev.buf("w"), wt, y, dev.ld["y"], m, kk, n, table if stats else None), want)
    out = y.download()
    assert poisoned(out) == 0, "y is not fully written"
    if not stats:
        assert untouched(table) == table.size
        return out, None
    t = table.download()
    assert poisoned(t) == 0 and np.isfinite(t).all(), "a row of the statistics table was not written"
    return out, t.astype(np.float64).sum(axis=0)


def bwd_data(ctx, dev, gview, residual, accumulate, want, own=None):
    m, kk, n = dev.k.shape
    dx = dev.fresh("dx")
    if accumulate:
        dx.upload(dev.k.base)
    res = (dev.buf("res"), dev.ld["r"]) if residual else (None, 0)
    run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_data", dev.gview(gview, own), dev.ld["y"], dev.buf("w"), dx, dev.ld["dx"], m, kk, n, res[0], res[1],
                              accumulate), want)
    out = dx.download()
    assert poisoned(out) == 0, "dx is not fully written"
    return out


def bwd_weight(ctx, dev, view, gview, want, defer=False):
    m, kk, n = dev.k.shape
    dw = dev.fresh("dW")
    call = lambda: ctx.call("ssdseg_pwconv_bwd_weight", dev.view(view), dev.ld["x"], dev.gview(gview), dev.ld["y"], dw, m, kk, n)     # noqa: E731
    if defer:
        ctx.colsum_defer(True)
        try:
            call()
            ctx.join()
        finally:
            ctx.colsum_defer(False)
    else:
        run(ctx, call, want)
    out = dw.download()
    assert poisoned(out) == 0, "dW is not fully written"
    return out


def bwd(ctx, dev, view, gview, residual, accumulate, want):
    m, kk, n = dev.k.shape
    dx, dw = dev.fresh("dx", "dW")
    if accumulate:
        dx.upload(dev.k.base)
    res = (dev.buf("res"), dev.ld["r"]) if residual else (None, 0)
    run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd", dev.view(view), dev.ld["x"], dev.gview(gview, own=view), dev.ld["y"], dev.buf("w"), dx, dev.ld["dx"],
                              dw, m, kk, n, res[0], res[1], accumulate), want)
    outs = dx.download(), dw.download()
    assert poisoned(outs[0]) == 0 and poisoned(outs[1]) == 0
    return outs


def bwd_bn(ctx, dev, view, gview, want):
    m, kk, n = dev.k.shape
    bufs = dev.fresh("dx", "dW", "dgamma", "dbeta", "k1out", "k0out")
    run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_bn", dev.view(view), dev.ld["x"], dev.gview(gview), dev.ld["y"], dev.buf("w"), bufs[0], dev.ld["dx"],
                              bufs[1], m, kk, n, dev.buf("mean"), dev.buf("invstd"), *bufs[2:]), want)
    outs = [b.download() for b in bufs]
    assert all(poisoned(o) == 0 for o in outs)
    return outs


# ------------------------------------------------------------------------------------------------------- lattice: bound 0
@pytest.mark.parametrize("name", list(P.CASES))
def test_lattice_is_exact_under_every_setting(ctx, guards, monkeypatch, name):
    """every form of every entry point the case names, under every setting it names: the launches are the mirror's, y, dx, dW, the
    row fold of the statistics and the fused dgamma / dbeta equal the float64 reference (bound 0), so the kernels equal each other;
    k1 / k0 within their rounding"""
    k = P.lattice_case(name)
    dev = Dev(ctx, guards, k)
    refs, first, kratio = {}, {}, 0.0

    def ref(key, make):
        if key not in refs:
            refs[key] = make()
        return refs[key]

    def same_as_first(key, setting, *arrays):
        kept = first.setdefault(key, (setting, [a + F32(0) for a in arrays]))
        for got, want in zip(arrays, kept[1]):
            assert same_bits(got + F32(0), want), (key, setting, "differs in bits from", kept[0])

    for setting in P.settings_of(name):
        use(monkeypatch, setting)
        for form in P.forms_of(name, "fwd"):
            view, stats = form
            y_ref, s_ref, q_ref = ref(("fwd", view), lambda: P.ref_fwd(k, view))
            y, fold = fwd(ctx, dev, view, stats, P.expected_launches(name, setting, "fwd", form)[0])
            what = (setting, "fwd", P.form_name(form))
            assert ratio(y, y_ref, 0.0) == 0.0, what
            same_as_first(("fwd", form), setting, y)
            if stats:
                assert ratio(fold[0], s_ref, 0.0) == 0.0 and ratio(fold[1], q_ref, 0.0) == 0.0, what
            if view == O.ACT_ZERO:
                assert not y.any(), what
        for form in P.forms_of(name, "bwd_data"):
            gview, residual, accumulate = form
            dx_ref = ref(("dx", form), lambda: P.ref_dx(k, gview, residual, accumulate))
            dx = bwd_data(ctx, dev, gview, residual, accumulate, P.expected_launches(name, setting, "bwd_data", form)[0])
            assert ratio(dx, dx_ref, 0.0) == 0.0, (setting, "bwd_data", P.form_name(form))
            same_as_first(("dx", form), setting, dx)
        for i, form in enumerate(P.forms_of(name, "bwd_weight")):
            view, gview = form
            dw_ref = ref(("dW", form), lambda: P.ref_dw(k, view, gview))
            dw = bwd_weight(ctx, dev, view, gview, P.expected_launches(name, setting, "bwd_weight", form)[0])
            assert ratio(dw, dw_ref, 0.0) == 0.0, (setting, "bwd_weight", P.form_name(form))
            same_as_first(("dW", form), setting, dw)
            if i == 0:
                deferred = bwd_weight(ctx, dev, view, gview, None, defer=True)
                assert same_bits(deferred + F32(0), dw + F32(0)), (setting, "bwd_weight with the column sum deferred")
        for form in P.forms_of(name, "bwd"):
            view, gview, residual, accumulate = form
            own = P.own_y(k, view)
            dx_ref, dw_ref = ref(("both", form), lambda: (P.ref_dx(k, gview, residual, accumulate, y=own), P.ref_dw(k, view, gview, y=own)))
            dx, dw = bwd(ctx, dev, view, gview, residual, accumulate, P.expected_launches(name, setting, "bwd", form)[0])
            what = (setting, "bwd", P.form_name(form))
            assert ratio(dx, dx_ref, 0.0) == 0.0 and ratio(dw, dw_ref, 0.0) == 0.0, what
            same_as_first(("both", form), setting, dx, dw)
        for form in P.forms_of(name, "bwd_bn"):
            view, gview = form
            r = ref(("bn", form), lambda: P.ref_bn(k, view, gview))
            dx, dw, dgamma, dbeta, k1, k0 = bwd_bn(ctx, dev, view, gview, P.expected_launches(name, setting, "bwd_bn", form)[0])
            for got, want in zip((dx, dw, dgamma, dbeta), r[:4]):
                assert ratio(got, want, 0.0) == 0.0, (setting, "bwd_bn", P.form_name(form))
            same_as_first(("bn", form), setting, dx, dw, dgamma, dbeta)
            kratio = max(kratio, ratio(k1, r[4], r[6][0] + 1e-300), ratio(k0, r[5], r[6][1] + 1e-300))
    RAN.add(name)
    report("pwconv", f"{name} [{k.mode}]", k1k0=kratio)


# ------------------------------------------------------------------------------------------------ normal: derived bounds
@pytest.mark.parametrize("name", P.NORMAL_CASES)
def test_normal_family_within_derived_bounds(ctx, guards, monkeypatch, name):
    k = P.normal_case(name)
    dev = Dev(ctx, guards, k)
    entries = P.CASES[name]["entries"]
    worst = {}

    def keep(launches, **ratios):
        kernel = sorted(s for s in launches if s.startswith(("gemm_", "pw_")))
        for q, v in ratios.items():
            key = f"{kernel[0].split('<')[0] if q != 'dW' else kernel[-1].split('<')[0]}:{q}"
            worst[key] = max(worst.get(key, 0.0), v)

    for setting in P.settings_of(name):
        use(monkeypatch, setting)
        for view, gview, residual, accumulate in ((O.ACT_RELU6, O.ACT_RELU6, 1, 1), ("plain", "identity", 0, 0), (O.ACT_NONE, O.ACT_RELU, 0, 1)):
            b = P.normal_bounds(k, view, gview, residual, accumulate)
            if "fwd" in entries:
                want = P.expected_launches(name, setting, "fwd", (view, True))[0]
                y_ref, s_ref, q_ref = P.ref_fwd(k, view)
                y, fold = fwd(ctx, dev, view, True, want)
                keep(want, y=ratio(y, y_ref, b["y"]), sum=ratio(fold[0], s_ref, b["sum"]), sumsq=ratio(fold[1], q_ref, b["sumsq"]))
            if "bwd_data" in entries:
                want = P.expected_launches(name, setting, "bwd_data", (gview, residual, accumulate))[0]
                dx = bwd_data(ctx, dev, gview, residual, accumulate, want)
                keep(want, dx=ratio(dx, P.ref_dx(k, gview, residual, accumulate), b["dx"]))
            if "bwd_weight" in entries:
                want = P.expected_launches(name, setting, "bwd_weight", (view, gview))[0]
                keep(want, dW=ratio(bwd_weight(ctx, dev, view, gview, want), P.ref_dw(k, view, gview), b["dW"]))
            if "bwd" in entries:
                # (the identity gradient view: a recomputed y off the lattice could flip a mask the stored one does not)
                bi = P.normal_bounds(k, view, "identity", residual, accumulate)
                want = P.expected_launches(name, setting, "bwd", (view, "identity", residual, accumulate))[0]
                dx, dw = bwd(ctx, dev, view, "identity", residual, accumulate, want)
                keep(want, dx=ratio(dx, P.ref_dx(k, "identity", residual, accumulate), bi["dx"]), dW=ratio(dw, P.ref_dw(k, view, "identity"), bi["dW"]))
            if "bwd_bn" in entries and view != "plain":
                b0 = P.normal_bounds(k, view, gview)
                want = P.expected_launches(name, setting, "bwd_bn", (view, gview))[0]
                r = P.ref_bn(k, view, gview)
                dx, dw, dgamma, dbeta, k1, k0 = bwd_bn(ctx, dev, view, gview, want)
                keep(want, dx=ratio(dx, r[0], b0["dx"]), dW=ratio(dw, r[1], b0["dW"]), dgamma=ratio(dgamma, r[2], b0["dgamma"]),
                     dbeta=ratio(dbeta, r[3], b0["dbeta"]))
    report("pwconv-normal", name, **worst)


# ------------------------------------------------------------------------------------------------------------- unaligned
@pytest.mark.parametrize("name", list(P.UNALIGNED))
def test_unaligned_outputs_take_the_scalar_epilogue_with_the_same_values(ctx, guards, monkeypatch, name):
    """product behaviour, not a switch: a y, dx or residual that is offset by one float or has an odd pitch leaves through the scalar
    epilogue (EP = 0 in the symbol); ssdseg_pwconv_bwd_bn with a dx that is offset by one float runs the plain GEMM plus the reduction
    of ssdseg_bn_bwd_reduce (an odd lddx is a rejected call there: test_argument_contracts).  Same values as the aligned call, bit for bit"""
    from ssdseglib import _hip as H
    k = P.lattice_case(name)
    m, kk, n = k.shape
    dev = Dev(ctx, guards, k)
    large = m >= 65000
    for setting in P.settings_of(name):
        env = use(monkeypatch, setting)
        if "fwd" in P.UNALIGNED[name]:
            view = O.ACT_RELU6
            y_ref = P.ref_fwd(k, view)[0]
            y0, _ = fwd(ctx, dev, view, False, P.plan_fwd(m, kk, n, kk, env)[0])
            want = P.plan_fwd(m, kk, n, kk, env, aligned=False)[0]
            assert all(", 0, 0, 0, 0>" in s for s in want if s.startswith("gemm_rowA")), want
            flat = guards.out((m + 1, n), name="y+1")            # (one row more: the body holds the m n floats from offset 1 on)
            run(ctx, lambda: ctx.call("ssdseg_pwconv_fwd_wt", dev.view(view), kk, dev.buf("w"), None, flat.view(1, (m, n)), n, m, kk, n, None), want)
            got = flat.download().ravel()
            assert poisoned(got[:1]) == 1 and poisoned(got[m * n + 1:]) == n - 1, (setting, "offset y: written outside its m n floats")
            assert same_bits(got[1:m * n + 1].reshape(m, n), y0) and ratio(y0, y_ref, 0.0) == 0.0, (setting, "offset y")
            odd = guards.out((m, n), ld=n + 1, name="y odd pitch")
            run(ctx, lambda: ctx.call("ssdseg_pwconv_fwd_wt", dev.view(view), kk, dev.buf("w"), None, odd, n + 1, m, kk, n, None), want)
            assert same_bits(odd.download(), y0), (setting, "odd-pitch y")
        if "bwd_data" in P.UNALIGNED[name]:
            gview = O.ACT_RELU6
            dx_ref = P.ref_dx(k, gview, 1, 1)
            dx0 = bwd_data(ctx, dev, gview, 1, 1, P.plan_bwd_data(m, kk, n, n, env, True, True)[0])
            assert ratio(dx0, dx_ref, 0.0) == 0.0
            want = P.plan_bwd_data(m, kk, n, n, env, True, True, aligned=False)[0]
            assert all(s.endswith(", 1, 0, 0, 0, 0>") for s in want if s.startswith("gemm_rowA")), want
            gv, w, res = dev.gview(gview), dev.buf("w"), dev.buf("res")
            flat = guards.out((m + 1, kk), name="dx+1")
            flat.upload(np.concatenate([np.zeros(1, F32), k.base.ravel(), np.zeros(kk - 1, F32)]).reshape(m + 1, kk))
            run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_data", gv, n, w, flat.view(1, (m, kk)), kk, m, kk, n, res, kk, 1), want)
            got = flat.download().ravel()
            assert not got[:1].any() and not got[m * kk + 1:].any(), (setting, "offset dx: written outside its m k floats")
            assert same_bits(got[1:m * kk + 1].reshape(m, kk), dx0), (setting, "offset dx")
            odd = guards.out((m, kk), ld=kk + 1, name="dx odd pitch")
            odd.upload(k.base)
            run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_data", gv, n, w, odd, kk + 1, m, kk, n, res, kk, 1), want)
            assert same_bits(odd.download(), dx0), (setting, "odd-pitch dx")
            if not large:
                shifted = guards.inp(np.concatenate([np.zeros(1, F32), k.res.ravel(), np.zeros(kk - 1, F32)]).reshape(m + 1, kk), name="res+1")
                dx = dev.fresh("dx").upload(k.base)
                run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_data", gv, n, w, dx, kk, m, kk, n, shifted.view(1, (m, kk)), kk, 1), want)
                assert same_bits(dx.download(), dx0), (setting, "offset residual")
            oddres = guards.inp(k.res, ld=kk + 1, name="res odd pitch")
            dx = dev.fresh("dx").upload(k.base)
            run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_data", gv, n, w, dx, kk, m, kk, n, oddres, kk + 1, 1), want)
            assert same_bits(dx.download(), dx0), (setting, "odd-pitch residual")
        if "bwd_bn" in P.UNALIGNED[name]:
            view, gview = O.ACT_RELU6, O.ACT_RELU6
            r = P.ref_bn(k, view, gview)
            aligned = bwd_bn(ctx, dev, view, gview, P.plan_bwd_bn(m, kk, n, kk, n, env, True)[0])
            want = P.plan_bwd_bn(m, kk, n, kk, n, env, True, aligned=False)[0]
            assert want.get("bn_bwd_partial_kernel") == 1 and not any(", 2, 0>" in s or ", 2, 1>" in s for s in want), want
            flat = guards.out((m + 1, kk), name="dx+1 (bn)")
            bufs = dev.fresh("dW", "dgamma", "dbeta", "k1out", "k0out")
            run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_bn", dev.view(view), kk, dev.gview(gview), n, dev.buf("w"), flat.view(1, (m, kk)), kk, bufs[0],
                                      m, kk, n, dev.buf("mean"), dev.buf("invstd"), *bufs[1:]), want)
            got = flat.download().ravel()
            assert poisoned(got[:1]) == 1 and poisoned(got[m * kk + 1:]) == kk - 1, (setting, "offset dx: written outside its m k floats")
            outs = [got[1:m * kk + 1].reshape(m, kk)] + [b.download() for b in bufs]
            for got, al, want_ref in zip(outs[:4], aligned[:4], r[:4]):
                assert ratio(got, want_ref, 0.0) == 0.0 and same_bits(got + F32(0), al + F32(0)), (setting, "bwd_bn with an offset dx")
            assert ratio(outs[4], r[4], r[6][0] + 1e-300) <= 1.0 and ratio(outs[5], r[5], r[6][1] + 1e-300) <= 1.0
    assert H is not None


# ---------------------------------------------------------------------------------------------------- transposed weights
@pytest.mark.parametrize("name,setting", P.TRANSPOSED)
def test_forward_with_a_transposed_weight_copy_gives_the_same_bits(ctx, guards, monkeypatch, name, setting):
    """ssdseg_pwconv_fwd_wt with a copy from ssdseg_transpose_batch equals the call that transposes for itself, bit for bit; the copy
    is ignored where another kernel runs"""
    k = P.lattice_case(name)
    m, kk, n = k.shape
    dev = Dev(ctx, guards, k)
    use(monkeypatch, setting)
    view = O.ACT_RELU6
    y_ref, s_ref, q_ref = P.ref_fwd(k, view)
    own_want = P.expected_launches(name, setting, "fwd", (view, True))[0]
    y0, fold0 = fwd(ctx, dev, view, True, own_want)
    wt = guards.out((n, kk), name="wt")
    table = guards.inp(np.array([[dev.buf("w").ptr, wt.ptr, kk, n]], dtype=np.int64), name="table")
    ctx.call("ssdseg_transpose_batch", table, 1, P.cdiv(kk, 32) * P.cdiv(n, 32), kk * n)
    assert np.array_equal(wt.download(), k.w.T)
    env = P.SETTINGS[setting]
    want = P.plan_fwd(m, kk, n, kk, env, wt_copy=True, stats=True)[0]
    tile = any(s.startswith("pw_tile_kernel") for s in want)
    assert ("conv3_transpose_w_kernel" in own_want) == tile and "conv3_transpose_w_kernel" not in want
    y1, fold1 = fwd(ctx, dev, view, True, want, wt=wt)
    assert same_bits(y1, y0) and np.array_equal(fold1, fold0)
    assert ratio(y1, y_ref, 0.0) == 0.0 and ratio(fold1[0], s_ref, 0.0) == 0.0 and ratio(fold1[1], q_ref, 0.0) == 0.0


# ----------------------------------------------------------------------------------------------------- argument contracts
def test_argument_contracts(ctx, guards, monkeypatch):
    """every bad call is rejected before any launch: nothing in the timing registry, the outputs still poison"""
    from ssdseglib import _hip as H
    use(monkeypatch, "default")
    name = "rows33-16x96"
    k = P.lattice_case(name)
    m, kk, n = k.shape
    dev = Dev(ctx, guards, k)
    x, w, y, dx, dw, table, res = (dev.buf(b) for b in ("x", "w", "y", "dx", "dW", "stats", "res"))
    bn_in, bn_out = (dev.buf("mean"), dev.buf("invstd")), tuple(dev.buf(b) for b in ("dgamma", "dbeta", "k1out", "k0out"))
    vin, gv = dev.view(O.ACT_RELU6), dev.gview(O.ACT_RELU6)
    half_views = [H.view(x, dev.buf("scale"), None, O.ACT_RELU6), H.view(x, None, dev.buf("shift"), O.ACT_RELU6), H.view(None)]

    def half_gview(missing):
        parts = dict(y=dev.buf("yraw"), scale=dev.buf("gscale"), shift=dev.buf("gshift"), k1=dev.buf("k1"), k0=dev.buf("k0"))
        parts[missing] = None
        return H.gview(dev.buf("g"), parts["y"], parts["scale"], parts["shift"], parts["k1"], parts["k0"], act=O.ACT_RELU6)

    def calls_of(vin=vin, gv=gv, w=w, y=y, dx=dx, dw=dw, m=m, k=kk, n=n, ldx=kk, ldy=n, lddx=kk, res=None, ldr=0, which="all", mean=bn_in[0],
                 invstd=bn_in[1], bn_out=bn_out):
        out = {"fwd": ("ssdseg_pwconv_fwd_wt", (vin, ldx, w, None, y, ldy, m, k, n, table)),
               "bwd_data": ("ssdseg_pwconv_bwd_data", (gv, ldy, w, dx, lddx, m, k, n, res, ldr, 0)),
               "bwd_weight": ("ssdseg_pwconv_bwd_weight", (vin, ldx, gv, ldy, dw, m, k, n)),
               "bwd": ("ssdseg_pwconv_bwd", (vin, ldx, gv, ldy, w, dx, lddx, dw, m, k, n, res, ldr, 0)),
               "bwd_bn": ("ssdseg_pwconv_bwd_bn", (vin, ldx, gv, ldy, w, dx, lddx, dw, m, k, n, mean, invstd) + tuple(bn_out))}
        return [out[e] for e in (out if which == "all" else which)]

    calls = []
    for bad in (dict(k=18, ldx=20, lddx=20), dict(k=0), dict(n=94, ldy=96), dict(n=0), dict(m=0), dict(m=-1)):
        calls += calls_of(**bad)
    calls += calls_of(ldx=kk - 4, which=("fwd", "bwd_weight", "bwd", "bwd_bn"))             # ldx < k
    calls += calls_of(ldx=kk + 2, which=("fwd", "bwd_weight", "bwd", "bwd_bn"))             # an input pitch that is not a multiple of 4
    calls += calls_of(ldy=n + 2, which=("bwd_data", "bwd_weight", "bwd", "bwd_bn"))
    calls += calls_of(ldy=n - 4)
    calls += calls_of(lddx=kk - 4, which=("bwd_data", "bwd", "bwd_bn"))
    # the fused BatchNorm form reads dx back as float4 rows (epilogue or reduction): an odd pitch is refused before the GEMM is launched
    calls += calls_of(lddx=kk + 1, which=("bwd_bn",)) + calls_of(lddx=kk + 2, which=("bwd_bn",))
    calls += calls_of(res=res, ldr=kk - 4, which=("bwd_data", "bwd"))
    for v in half_views:
        calls += calls_of(vin=v, which=("fwd", "bwd_weight", "bwd", "bwd_bn"))
    calls += calls_of(vin=None, which=("fwd", "bwd_weight", "bwd", "bwd_bn"))
    calls += calls_of(vin=dev.view("plain"), which=("bwd_bn",))                             # the fused sums need the BatchNorm's view
    for missing in ("y", "shift", "k1", "k0"):
        calls += calls_of(gv=half_gview(missing), which=("bwd_data", "bwd_weight", "bwd", "bwd_bn"))
    calls += calls_of(gv=H.gview(None), which=("bwd_data", "bwd_weight", "bwd", "bwd_bn"))
    calls += calls_of(gv=None, which=("bwd_data", "bwd_weight", "bwd", "bwd_bn"))
    calls += calls_of(w=None, which=("fwd", "bwd_data", "bwd", "bwd_bn"))
    calls += calls_of(y=None, which=("fwd",))
    calls += calls_of(dx=None, which=("bwd_data", "bwd", "bwd_bn"))
    calls += calls_of(dw=None, which=("bwd_weight", "bwd", "bwd_bn"))
    calls += calls_of(mean=None, which=("bwd_bn",)) + calls_of(invstd=None, which=("bwd_bn",))
    calls += calls_of(bn_out=bn_out[:2] + (None, bn_out[3]), which=("bwd_bn",)) + calls_of(bn_out=bn_out[:3] + (None,), which=("bwd_bn",))
    for entry, args in calls:
        kernels = launched(ctx, lambda: rejected(ctx, entry, *args))
        assert kernels == {}, (entry, kernels)
    for name_, dims in (("ssdseg_pwconv_parts", (0, n)), ("ssdseg_pwconv_parts", (m, 0)), ("ssdseg_pwconv_wt_floats", (0, kk, kk, n)),
                        ("ssdseg_pwconv_wt_floats", (m, kk, 0, n))):
        with pytest.raises(H.SsdsegError, match=f"{name_}: invalid argument"):
            ctx.parts(name_, *dims)
    for o in (y, dx, dw, table) + bn_out:
        assert untouched(o) == o.size
    # the good calls still run; dgamma / dbeta may be NULL
    want = P.expected_launches(name, "default", "bwd_bn", (O.ACT_RELU6, O.ACT_RELU6))[0]
    r = P.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6)
    dx_, dw_, dgamma, dbeta, k1, k0 = bwd_bn(ctx, dev, O.ACT_RELU6, O.ACT_RELU6, want)
    assert ratio(dx_, r[0], 0.0) == 0.0 and ratio(dgamma, r[2], 0.0) == 0.0
    bufs = dev.fresh("dx", "dW", "k1out", "k0out")
    run(ctx, lambda: ctx.call("ssdseg_pwconv_bwd_bn", vin, kk, gv, n, w, bufs[0], kk, bufs[1], m, kk, n, bn_in[0], bn_in[1], None, None, bufs[2], bufs[3]), want)
    assert same_bits(bufs[2].download(), k1) and same_bits(bufs[3].download(), k0) and ratio(bufs[0].download(), r[0], 0.0) == 0.0


# --------------------------------------------------------------------------------------------------------------- coverage
def test_the_suite_reaches_every_kernel_it_is_there_for():
    """the instantiations the cases exist for are among the launches the mirror names -- each lattice test asserts that what ran is
    exactly that -- and, when every case ran in this process, among what the timing registry recorded"""
    planned = P.planned_symbols()
    assert P.coverage_gaps(planned) == []
    if RAN >= set(P.CASES):
        assert P.coverage_gaps(RECORDED) == []
