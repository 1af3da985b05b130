"""GPU parity of the dense 3x3 conv kernels at their edges (through the C-ABI) vs float64.

ssdseg_conv3x3_parts / _saved_floats / _fwd / _fwd_saved / _fwd_saved_from / _bwd_weight_saved / _bwd_data / _bwd_data_bn / _bwd_weight
(csrc/conv3.hip and its headers, csrc/conv3n.hip, the implicit-GEMM paths of csrc/gemm.hip) on the cases of tests/_conv3_cases.py: one
pixel, one whole 8 x 32 pixel tile, ragged tile rows and columns next to another image's rows, odd sizes under F(2x2); every width of
the halo tile's column tiles in both roles; F(4x4) below, at and over a 4 x 4 tile, with tr != tc, two blocks along w, one and three
16-channel steps, its plain-store path; the implicit GEMM for channel counts the tiles refuse, the BatchNorm gradient view and row
tiles across image borders; the narrow form and its direct kernel at every pixel trip; the halo-tile, nine-tap, per-tap and Winograd
weight gradients at their split-K and even-deal edges; the saved-input pair with c_from > 0 -- each under the switch settings that
change its kernel (set per call with monkeypatch, every SSDSEG_CONV3_* / SSDSEG_CONV3N_DIRECT / SSDSEG_W4_* and pointwise switch
cleared first), each form of the two views.  tests/test_cpu_conv3_cases.py vets the reference, the cases and the mirror.  Every buffer
is guarded (tests/_guard.py); the launches are read from the timing registry and the kernel the setting is there for must be among them.

Bounds.  U = 2^-24, gamma(L) = L U / (1 - L U).

  lattice family   0 for y, dx (overwrite, accumulate, into a channel slice), dW, the float64 fold of the statistics rows to sum y and
                   the fused dgamma / dbeta of ssdseg_conv3x3_bwd_data_bn: the inputs are small multiples of powers of two and every
                   reduction stays below 2^24 units of its lattice (_conv3_cases.budget), the transformed domains of F(2x2, 3x3) and
                   of the Winograd weight gradient included (their matrices hold 0, +-1, 1/2: additions and exact halvings), so
                   float32 arithmetic is exact in any order and every kernel must give the same numbers: each result is also compared
                   bit for bit with the first setting's, after x + 0 on both.  sum y^2: 0 where its budget holds too, else
                   gamma(M + 2) sum y^2, M = n h w.  k1, k0: U |k| + 2^-50 of the absolute terms of their formulas (the finalize
                   kernel works in float64 from the exact sums and rounds once).
  F(4x4, 3x3)      exact in neither family: G holds 1/6, 1/12, 1/24, B^T and A^T constants up to 8.  Roundings on the longest path of
                   a 1-D pass, per row of the matrix, from csrc/conv3_wino4.h.  G (conv3_wino4_weights_kernel, contracted to
                   multiply-adds): row 0 one multiply; rows 1, 2 add, add, multiply = 3; rows 3, 4 multiply, fma, fma = 3; row 5
                   none; rows 1 .. 4 also carry a rounded constant: [1, 3, 3, 3, 3, 0] + [0, 1, 1, 1, 1, 0].  B^T (w4_bt_lo /
                   w4_bt_hi): row 0 = fma(4, d0, (fma(-4, d2, d4) - d2)) = 3, every other row one operation on two one-operation
                   terms = 2: [3, 2, 2, 2, 2, 2].  A^T (epilogue_round): rows 0 and 3 three dependent operations, rows 1 and 2 a
                   subtraction or sum, then one fma = 2: [3, 2, 2, 3].  The worst path through U, the view, V and the output is
                   r = 6 + 1 + 6 + 6 = 19 and gives the worst-path bound
                       (gamma(cred + r) + 3 . 2U) |A^T| [ sum_c (|G||w_c||G^T|) . (|B^T||d_c||B|) ] |A|
                   of which the emulation and the kernel stay below 0.01.  So the tests hold both to the per-position form, which it
                   dominates: with eu, ev, ey the counts above per POSITION (row + column, + 1 in ev under a view) times U,
                       |A^T| [ sum_c ( eu . U'_c . |V_c| + ev . |U_c| . V'_c + gamma(cred) |U_c| . |V_c| ) ] |A| + ey . |A^T| |M| |A|
                   (U', V': the |.|-matrix forms; M = sum_c U_c . V_c; (1 + 2^-10) for the products of two errors).  The MFMA chain
                   adds cred exact products: at most cred roundings in any order.  An accumulating input gradient adds one rounding
                   of the running total.  Statistics: gamma(M + 1) sum |y| + sum b; gamma(M + 2) sum y^2 + sum (2 |y| b + b^2).
  normal family    any-order bounds.  a = act(s x + t) is one fused multiply-add: |da| <= U A, A = |s x| + |t| >= |a|.
                   y: 9 cin exact products summed in some order + the view's rounding: (gamma(9 cin + 1) + U) sum A |w| -- the tap-
                   expanded narrow form (cin products, then nine taps) and the direct kernel's 36-term chain stay inside it.
                   dy = s m g + (k1 y + k0): two roundings of D = |s g| + |k1 y| + |k0| (identity: D = |g|, exact); the mask is safe:
                   |z| U < 1e-6 << the 1e-4 band.  dx: (gamma(9 cout + 1) + 2 U) sum D |w|, + one rounding of the total when it
                   accumulates.  dW: a float32 chain of at most M terms, the slab sum, one rounding: (gamma(M + 2) + 3 U) sum A D +
                   gamma(2) |dW|.  F(2x2): additions and exact halvings: gamma(cred + 11) |A^T| [sum_c U' . V'] |A| (4 for U, 1 for
                   the view, 2 for V, 4 for the output); its weight gradient gamma(tiles + slots + 9) |G^T| [sum_tiles V' . Z'] |G|.
                   Fused sums: gamma(M + 1) sum |m dx| + sum of the dx bounds, the same with |xhat| and 2 U for xhat's two roundings,
                   + one rounding of the result.

ssdseg_conv3x3_bwd_data and a dx pitch that is no multiple of 4 (the other entry points refuse one): every family it reaches stores
dx four bytes at a time -- conv3_tile.h:217, conv3_wino.h:304, conv3_wino4.h:411 / :419 (raw_buffer_store_b32), the implicit GEMM's
scalar epilogue (LD = 1 never takes the float4 one, gemm.hip launch_rowA), the narrow form's pointwise GEMM (pw_tile.h:254;
launch_rowA tests ldo % 4 before its float4 epilogue; from 500,000 rows gemm_wres_kernel, gemm_wres.h:219-221); the direct kernel's
16-byte stores belong to ssdseg_conv3x3_bwd_data_bn, which checks.  So no check is missing: test_input_gradient_into_an_odd_pitch
runs such calls and demands the same bits.

Run with -s for the largest error / bound ratio of every case (DESIGN.md records them).
"""
import ctypes as C
import re

import numpy as np
import pytest

import _conv3_cases as P
from oracle import np_ops as O
from _guard import BODY_WORD, guards  # noqa: F401  (fixture)
from _edge_helpers import launched, ratio, reporter, same_bits, untouched

pytestmark = pytest.mark.gpu

F32 = np.float32
report = reporter("conv3-edges")
RECORDED = set()        # every kernel symbol the timing registry showed in this process
RAN = set()             # the lattice cases that ran in this process
POISON = np.array([BODY_WORD], np.uint32).view(F32)[0]


@pytest.fixture(scope="module")
def cus(ctx):
    """the device's CU count (the split-K and even-deal arithmetic of the weight gradients is sized by it) as the library itself holds
    it: ssdseg_ctx_device_name ends in "N CUs)" """
    count = re.search(r"(\d+) CUs\)$", ctx.device_name())
    assert count and int(count.group(1)) > 0, ctx.device_name()
    return int(count.group(1))


def use(monkeypatch, setting):
    for v in P.CONV3_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, value in P.SETTINGS[setting].items():
        monkeypatch.setenv(v, value)
    return P.SETTINGS[setting]


def poisoned(a):
    return int((np.ascontiguousarray(a).view(np.uint32) == np.uint32(BODY_WORD)).sum())


def run(ctx, fn, pattern):
    """the launches of fn(): the kernel the setting is there for is among them"""
    kernels = launched(ctx, fn)
    RECORDED.update(kernels)
    assert P.reaches(kernels, pattern), ("launched", kernels, "expected one matching", pattern)
    return kernels


class Dev:
    """the operands of one case on the device, guarded, x and dx at the case's row pitch; allocated when first used"""

    def __init__(self, ctx, guards, k):
        self.ctx, self.guards, self.k = ctx, guards, k
        self._bufs = {}

    def buf(self, name):
        if name not in self._bufs:
            k, g = self.k, self.guards
            n, h, w, cin, cout = k.shape
            m = n * h * w
            if name == "x":
                b = g.inp(k.x.reshape(m, cin), ld=k.ldx, name=name)
            elif name in ("g", "yraw"):
                b = g.inp(getattr(k, name).reshape(m, cout), name=name)
            elif name == "y":
                b = g.out((m, cout), name=name)
            elif name == "dx":
                b = g.out((m, cin), ld=k.ldx, name=name)
            elif name == "wide":
                b = g.out((m, cin + 8), name=name)
            elif name == "dW":
                b = g.out((3, 3, cin, cout), name=name)
            elif name in ("dgamma", "dbeta", "k1out", "k0out"):
                b = g.out((cin,), name=name)
            elif name == "stats":
                b = g.out((self.ctx.parts("ssdseg_conv3x3_parts", n, h, w, cin, cout), 2, cout), name=name)
            else:
                b = g.inp(getattr(k, name), name=name)
            self._bufs[name] = b
        return self._bufs[name]

    def view(self, view):
        from ssdseglib import _hip as H
        return H.view(self.buf("x")) if view == "plain" else H.view(self.buf("x"), self.buf("scale"), self.buf("shift"), view)

    def gview(self, gview):
        from ssdseglib import _hip as H
        if gview == "identity":
            return H.gview(self.buf("g"))
        return H.gview(self.buf("g"), self.buf("yraw"), self.buf("gscale"), self.buf("gshift"), self.buf("k1"), self.buf("k0"), act=gview)

    def fresh(self, *names):
        out = [self.guards.repoison(self.buf(nm)) for nm in names]
        return out if len(out) > 1 else out[0]


def fwd(ctx, dev, view, stats, pattern):
    """-> (y, float64 fold of the statistics rows or None)"""
    k = dev.k
    n, h, w, cin, cout = k.shape
    y, table = dev.fresh("y", "stats")
    run(ctx, lambda: ctx.call("ssdseg_conv3x3_fwd", dev.view(view), k.ldx, dev.buf("w"), y, n, h, w, cin, cout, table if stats else None), pattern)
    out = y.download().reshape(n, h, w, cout)
    assert poisoned(out) == 0, "y is not fully written"
    if not stats:
        assert untouched(table) == table.size
        return out, None
    t = table.download()
    assert poisoned(t) == 0 and np.isfinite(t).all(), "a row of the statistics table was neither written nor zeroed"
    return out, t.astype(np.float64).sum(axis=0)


def bwd_data(ctx, dev, gview, accumulate, sliced, pattern):
    k = dev.k
    n, h, w, cin, cout = k.shape
    m = n * h * w
    if sliced:
        # channels 4 .. 4 + cin of a wider (concat) gradient buffer; the channels beside the slice keep the poison
        wide = dev.fresh("wide")
        if accumulate:
            host = np.full((m, cin + 8), POISON, F32)
            host[:, 4:4 + cin] = k.base.reshape(m, cin)
            wide.upload(host)
        run(ctx, lambda: ctx.call("ssdseg_conv3x3_bwd_data", dev.gview(gview), dev.buf("w"), wide.view(4, (wide.size - 4,)), cin + 8, n, h, w, cin, cout,
                                  accumulate), pattern)
        got = wide.download()
        assert poisoned(got[:, :4]) == 4 * m and poisoned(got[:, 4 + cin:]) == 4 * m, "written beside the channel slice"
        out = got[:, 4:4 + cin]
    else:
        dx = dev.fresh("dx")
        if accumulate:
            dx.upload(k.base.reshape(m, cin))
        run(ctx, lambda: ctx.call("ssdseg_conv3x3_bwd_data", dev.gview(gview), dev.buf("w"), dx, k.ldx, n, h, w, cin, cout, accumulate), pattern)
        out = dx.download()
    assert poisoned(out) == 0, "dx is not fully written"
    return np.ascontiguousarray(out).reshape(n, h, w, cin)


def bwd_data_bn(ctx, dev, view, gview, pattern):
    k = dev.k
    n, h, w, cin, cout = k.shape
    bufs = dev.fresh("dx", "dgamma", "dbeta", "k1out", "k0out")
    run(ctx, lambda: ctx.call("ssdseg_conv3x3_bwd_data_bn", dev.view(view), dev.gview(gview), dev.buf("w"), bufs[0], k.ldx, n, h, w, cin, cout,
                              dev.buf("mean"), dev.buf("invstd"), *bufs[1:]), pattern)
    outs = [b.download() for b in bufs]
    assert all(poisoned(o) == 0 for o in outs)
    return [outs[0].reshape(n, h, w, cin)] + outs[1:]


def bwd_weight(ctx, dev, view, gview, pattern):
    k = dev.k
    n, h, w, cin, cout = k.shape
    dw = dev.fresh("dW")
    run(ctx, lambda: ctx.call("ssdseg_conv3x3_bwd_weight", dev.view(view), k.ldx, dev.gview(gview), dw, n, h, w, cin, cout), pattern)
    out = dw.download()
    assert poisoned(out) == 0, "dW is not fully written"
    return out


def stats_ratios(k, fold, y_ref, y_b, sumsq_exact):
    """sum y and sum y^2 of the folded table against the reference: y_b None = y is exact"""
    m = k.shape[0] * k.shape[1] * k.shape[2]
    s_ref, q_ref = y_ref.sum(axis=(0, 1, 2)), (y_ref * y_ref).sum(axis=(0, 1, 2))
    if y_b is None:
        assert ratio(fold[0], s_ref, 0.0) == 0.0, "the fold of the statistics rows is not sum y"
        if sumsq_exact:
            assert ratio(fold[1], q_ref, 0.0) == 0.0, "the fold of the statistics rows is not sum y^2"
            return 0.0, 0.0
        return 0.0, ratio(fold[1], q_ref, P.gamma(m + 2) * q_ref + 1e-300)
    s_b = P.gamma(m + 1) * np.abs(y_ref).sum(axis=(0, 1, 2)) + y_b.sum(axis=(0, 1, 2))
    return ratio(fold[0], s_ref, s_b + 1e-300), ratio(fold[1], q_ref, P.sumsq_bound(y_ref, y_b) + 1e-300)


# ------------------------------------------------------------------------------------------------------- lattice: bound 0
@pytest.mark.parametrize("name", [nm for nm in P.CASES if nm not in P.SAVED])
def test_lattice_is_exact_under_every_setting(ctx, guards, monkeypatch, cus, name):
    """every form of every entry point the case names, under every setting it names: the kernel the setting is there for ran; y, dx,
    dW, the fold of the statistics rows and the fused dgamma / dbeta equal the float64 reference (bound 0), so the kernels equal each
    other; F(4x4) within its derived bound; k1 / k0 within their rounding"""
    k = P.lattice_case(name)
    dev = Dev(ctx, guards, k)
    first, worst = {}, dict(k1k0=0.0, f4=0.0, sumsq=0.0)
    sumsq_exact = P.budget(k)["sumsq"] < P.EXACT

    def same_as_first(key, setting, *arrays):
        kept = first.setdefault(key, (setting, [a + F32(0) for a in arrays]))
        for got, want in zip(arrays, kept[1]):
            assert same_bits(got + F32(0), want), (key, setting, "differs in bits from", kept[0])

    for setting in P.settings_of(name):
        use(monkeypatch, setting)
        for form in P.forms_of(name, "fwd"):
            view, stats = form
            what = (setting, "fwd", P.form_name(form))
            f4 = P.plan_of(name, setting, "fwd", form)["family"] == "wino4"
            y_ref = P.ref_fwd(k, view)[0]
            y_b = P.f4_bound_fwd(k, view) if f4 else None
            y, fold = fwd(ctx, dev, view, stats, P.expected_kernel(name, setting, "fwd", form, cus))
            if f4:
                worst["f4"] = max(worst["f4"], ratio(y, y_ref, y_b))
            else:
                assert ratio(y, y_ref, 0.0) == 0.0, what
            same_as_first(("fwd", form), setting, y)
            if stats:
                rs, rq = stats_ratios(k, fold, y_ref, y_b, sumsq_exact)
                worst["f4"], worst["sumsq"] = max(worst["f4"], rs), max(worst["sumsq"], rq)
            if view == O.ACT_ZERO:
                assert not y.any(), what
        for form in P.forms_of(name, "bwd_data"):
            gview, accumulate, sliced = form
            f4 = P.plan_of(name, setting, "bwd_data", form)["family"] == "wino4"
            dx = bwd_data(ctx, dev, gview, accumulate, sliced, P.expected_kernel(name, setting, "bwd_data", form, cus))
            if f4:
                worst["f4"] = max(worst["f4"], ratio(dx, P.ref_dx(k, gview, accumulate), P.f4_bound_dx(k, accumulate)))
            else:
                assert ratio(dx, P.ref_dx(k, gview, accumulate), 0.0) == 0.0, (setting, "bwd_data", P.form_name(form))
            same_as_first(("dx", form), setting, dx)
        for form in P.forms_of(name, "bwd_data_bn"):
            view, gview = form
            r = P.ref_bn(k, view, gview)
            dx, dgamma, dbeta, k1, k0 = bwd_data_bn(ctx, dev, view, gview, P.expected_kernel(name, setting, "bwd_data_bn", form, cus))
            for got, want in zip((dx, dgamma, dbeta), r[:3]):
                assert ratio(got, want, 0.0) == 0.0, (setting, "bwd_data_bn", P.form_name(form))
            same_as_first(("bn", form), setting, dx, dgamma, dbeta)
            worst["k1k0"] = max(worst["k1k0"], ratio(k1, r[3], r[5][0] + 1e-300), ratio(k0, r[4], r[5][1] + 1e-300))
        for form in P.forms_of(name, "bwd_weight"):
            view, gview = form
            dw = bwd_weight(ctx, dev, view, gview, P.expected_kernel(name, setting, "bwd_weight", form, cus))
            assert ratio(dw, P.ref_dw(k, view, gview), 0.0) == 0.0, (setting, "bwd_weight", P.form_name(form))
            same_as_first(("dW", form), setting, dw)
    RAN.add(name)
    report("conv3x3", f"{name} [{k.mode}]", **worst)


# ------------------------------------------------------------------------------------------------ normal: derived bounds
def dx_bound(k, family, gview, accumulate, b):
    """the bound of dx under the family that computes it (a Winograd form only ever sees the plain gradient)"""
    if family not in ("wino", "wino4"):
        return b["dx"]
    if family == "wino4":
        return P.f4_bound_dx(k, accumulate)
    dx_b = P.f2_bound(np.abs(k.g.astype(np.float64)), P.flipped(k.w.astype(np.float64)), k.shape[4])
    return dx_b + P.U * (np.abs(P.ref_dx(k, gview)) + dx_b + np.abs(k.base)) if accumulate else dx_b


@pytest.mark.parametrize("name", P.NORMAL_CASES)
def test_normal_family_within_derived_bounds(ctx, guards, monkeypatch, cus, name):
    k = P.normal_case(name)
    n, h, w, cin, cout = k.shape
    dev = Dev(ctx, guards, k)
    entries = P.CASES[name]["entries"]
    worst = {}

    def keep(family, **ratios):
        for q, v in ratios.items():
            worst[f"{family}:{q}"] = max(worst.get(f"{family}:{q}", 0.0), v)

    for setting in P.settings_of(name):
        use(monkeypatch, setting)
        for view, gview, accumulate in ((O.ACT_RELU6, O.ACT_RELU6, 1), ("plain", "identity", 0), (O.ACT_NONE, "identity", 1)):
            b = P.normal_bounds(k, view, gview, accumulate)
            if "fwd" in entries:
                form = (view, True)
                fam = P.plan_of(name, setting, "fwd", form)["family"]
                y_ref = P.ref_fwd(k, view)[0]
                y_b = P.f4_bound_fwd(k, view) if fam == "wino4" else (P.f2_bound(P.view_abs(k, view), k.w.astype(np.float64), cin) if fam == "wino" else b["y"])
                y, fold = fwd(ctx, dev, view, True, P.expected_kernel(name, setting, "fwd", form, cus))
                rs, rq = stats_ratios(k, fold, y_ref, y_b, False)
                keep(fam, y=ratio(y, y_ref, y_b), sum=rs, sumsq=rq)
            if "bwd_data" in entries:
                form = (gview, accumulate, False)
                fam = P.plan_of(name, setting, "bwd_data", form)["family"]
                dx = bwd_data(ctx, dev, gview, accumulate, False, P.expected_kernel(name, setting, "bwd_data", form, cus))
                keep(fam, dx=ratio(dx, P.ref_dx(k, gview, accumulate), dx_bound(k, fam, gview, accumulate, b)))
            if "bwd_data_bn" in entries and view != "plain":
                form = (view, gview)
                fam = P.plan_of(name, setting, "bwd_data_bn", form)["family"]
                b0 = P.normal_bounds(k, view, gview)
                b0 = P.normal_bounds(k, view, gview, dx_b=dx_bound(k, fam, gview, 0, b0))
                r = P.ref_bn(k, view, gview)
                dx, dgamma, dbeta, k1, k0 = bwd_data_bn(ctx, dev, view, gview, P.expected_kernel(name, setting, "bwd_data_bn", form, cus))
                keep(fam, dx=ratio(dx, r[0], b0["dx"]), dgamma=ratio(dgamma, r[1], b0["dgamma"]), dbeta=ratio(dbeta, r[2], b0["dbeta"]))
            if "bwd_weight" in entries:
                form = (view, gview)
                p = P.plan_of(name, setting, "bwd_weight", form, cus)
                dw_b = P.f2_wgrad_bound(k, view, p["slots"]) if p["family"] == "wino" else b["dW"]
                dw = bwd_weight(ctx, dev, view, gview, P.expected_kernel(name, setting, "bwd_weight", form, cus))
                keep("w-" + p["family"], dW=ratio(dw, P.ref_dw(k, view, gview), dw_b))
    report("conv3x3-normal", name, **worst)


# ---------------------------------------------------------------------------------------------------- the saved-input pair
@pytest.mark.parametrize("name", list(P.SAVED))
def test_saved_input_pair_from_a_channel_offset(ctx, guards, monkeypatch, cus, name):
    """ssdseg_conv3x3_fwd_saved_from with c_from in {0, 4, cin - 4} and ldx > cin: the zero-bordered copy element by element (values in
    [c_from, cin), the pre-filled channels untouched, the border zero); y and the statistics bit-equal to ssdseg_conv3x3_fwd on the full
    view; ssdseg_conv3x3_bwd_weight_saved on that copy bit-equal to ssdseg_conv3x3_bwd_weight"""
    k = P.lattice_case(name)
    n, h, w, cin, cout = k.shape
    setting = P.settings_of(name)[0]
    env = use(monkeypatch, setting)
    dev = Dev(ctx, guards, k)
    need = C.c_longlong()
    assert ctx.lib.ssdseg_conv3x3_saved_floats(n, h, w, cin, cout, C.byref(need)) == 0 and need.value == P.saved_floats(env, n, h, w, cin, cout) > 0
    view = O.ACT_RELU6
    fam = P.fwd_plan(env, n, h, w, cin, cin, cout)["family"]
    y_ref = P.ref_fwd(k, view)[0]
    y_b = P.f4_bound_fwd(k, view) if fam == "wino4" else None
    y0, _ = fwd(ctx, dev, view, True, P.kernel_for("fwd", dict(family=fam), True))
    table0 = dev.buf("stats").download()
    dw0 = bwd_weight(ctx, dev, view, "identity", r"^conv3_wino_wgrad_kernel$")
    assert ratio(dw0, P.ref_dw(k, view, "identity"), 0.0) == 0.0
    worst = 0.0
    xs = guards.out((n, h + 2, w + 2, cin), name="xsaved")
    for c_from in P.c_froms(name):
        before, want = P.saved_copy(k, view, c_from, POISON)
        xs.upload(before)
        y, table = dev.fresh("y", "stats")
        kernels = run(ctx, lambda: ctx.call("ssdseg_conv3x3_fwd_saved_from", dev.view(view), k.ldx, dev.buf("w"), y, n, h, w, cin, cout, table, xs, c_from),
                      P.kernel_for("fwd", dict(family=fam), False))
        assert kernels.get("conv3_pad_view_kernel") == 1, kernels
        copy = xs.download()
        assert same_bits(copy[..., :c_from], before[..., :c_from]), (c_from, "the pre-filled channels were written")
        assert same_bits(copy + F32(0), want + F32(0)), (c_from, "the zero-bordered copy", np.argwhere(copy != want)[:4])
        y1 = y.download().reshape(n, h, w, cout)
        assert same_bits(y1, y0) and same_bits(table.download(), table0), (c_from, "y / statistics differ from ssdseg_conv3x3_fwd")
        if y_b is None:
            assert ratio(y1, y_ref, 0.0) == 0.0
        else:
            worst = max(worst, ratio(y1, y_ref, y_b))
        dw = dev.fresh("dW")
        run(ctx, lambda: ctx.call("ssdseg_conv3x3_bwd_weight_saved", xs, dev.buf("g"), dw, n, h, w, cin, cout), r"^conv3_wino_wgrad_kernel$")
        assert same_bits(dw.download(), dw0), (c_from, "dW differs from ssdseg_conv3x3_bwd_weight")
    # ssdseg_conv3x3_fwd_saved is c_from = 0
    xs.upload(P.saved_copy(k, view, 0, POISON)[0])
    y = dev.fresh("y")
    run(ctx, lambda: ctx.call("ssdseg_conv3x3_fwd_saved", dev.view(view), k.ldx, dev.buf("w"), y, n, h, w, cin, cout, None, xs), r"^conv3_pad_view_kernel$")
    assert same_bits(y.download().reshape(n, h, w, cout), y0) and same_bits(xs.download() + F32(0), P.saved_copy(k, view, 0)[1] + F32(0))
    report("conv3x3-saved", name, f4=worst)


# ------------------------------------------------------------------------------------------------------------- odd pitch
@pytest.mark.parametrize("name,setting", [("not-narrow-24x8", "default"), ("px-9x33", "wino"), ("f4-plain", "wino4"), ("f4-plain", "wino4-plain"),
                                          ("gemm-cout12", "default"), ("narrow-32x8", "default"), ("narrow-16x4", "default")])
def test_input_gradient_into_an_odd_pitch(ctx, guards, monkeypatch, cus, name, setting):
    """ssdseg_conv3x3_bwd_data takes a dx pitch that is no multiple of 4 (module docstring: every family it reaches stores four bytes at
    a time): the same bits as at the dense pitch, overwrite and accumulate, the gap column untouched (the guards' teardown check)"""
    k = P.lattice_case(name)
    n, h, w, cin, cout = k.shape
    m = n * h * w
    use(monkeypatch, setting)
    dev = Dev(ctx, guards, k)
    for accumulate in (0, 1):
        form = ("identity", accumulate, False)
        pattern = P.expected_kernel(name, setting, "bwd_data", form, cus)
        dense = bwd_data(ctx, dev, "identity", accumulate, False, pattern)
        odd = guards.out((m, cin), ld=cin + 1, name="dx odd pitch")
        if accumulate:
            odd.upload(k.base.reshape(m, cin))
        run(ctx, lambda: ctx.call("ssdseg_conv3x3_bwd_data", dev.gview("identity"), dev.buf("w"), odd, cin + 1, n, h, w, cin, cout, accumulate), pattern)
        got = odd.download().reshape(n, h, w, cin)
        assert poisoned(got) == 0 and same_bits(got, dense), (accumulate, "odd-pitch dx")


# ----------------------------------------------------------------------------------------------------- argument contracts
def test_argument_contracts(ctx, guards, monkeypatch):
    """every SSDSEG_ARG of the nine entry points: rejected before any launch -- nothing in the timing registry, the outputs still poison"""
    from ssdseglib import _hip as H
    name = "saved-f2"
    use(monkeypatch, P.settings_of(name)[0])
    k = P.lattice_case(name)
    n, h, w, cin, cout = k.shape
    dev = Dev(ctx, guards, k)
    x, wgt, y, dx, dw, table = (dev.buf(b) for b in ("x", "w", "y", "dx", "dW", "stats"))
    bn_in, bn_out = (dev.buf("mean"), dev.buf("invstd")), tuple(dev.buf(b) for b in ("dgamma", "dbeta", "k1out", "k0out"))
    xs = guards.out((n, h + 2, w + 2, cin), name="xsaved")
    vin, gv, g = dev.view(O.ACT_RELU6), dev.gview(O.ACT_RELU6), dev.buf("g")
    half_views = [H.view(x, dev.buf("scale"), None, O.ACT_RELU6), H.view(x, None, dev.buf("shift"), O.ACT_RELU6), H.view(None), None]

    def half_gview(missing):
        parts = dict(y=dev.buf("yraw"), scale=dev.buf("gscale"), shift=dev.buf("gshift"), k1=dev.buf("k1"), k0=dev.buf("k0"))
        parts[missing] = None
        return H.gview(g, parts["y"], parts["scale"], parts["shift"], parts["k1"], parts["k0"], act=O.ACT_RELU6)

    half_gviews = [half_gview(mi) for mi in ("y", "shift", "k1", "k0")] + [H.gview(None), None]

    def calls_of(which, vin=vin, gv=gv, wgt=wgt, y=y, dx=dx, dw=dw, xs=xs, g=g, dims=(n, h, w), cin=cin, cout=cout, ldx=k.ldx, c_from=4, mean=bn_in[0],
                 invstd=bn_in[1], bn_out=bn_out):
        d = tuple(dims) + (cin, cout)
        out = {"fwd": ("ssdseg_conv3x3_fwd", (vin, ldx, wgt, y) + d + (table,)),
               "fwd_saved": ("ssdseg_conv3x3_fwd_saved", (vin, ldx, wgt, y) + d + (table, xs)),
               "fwd_saved_from": ("ssdseg_conv3x3_fwd_saved_from", (vin, ldx, wgt, y) + d + (table, xs, c_from)),
               "bwd_weight_saved": ("ssdseg_conv3x3_bwd_weight_saved", (xs, g, dw) + d),
               "bwd_data": ("ssdseg_conv3x3_bwd_data", (gv, wgt, dx, ldx) + d + (0,)),
               "bwd_data_bn": ("ssdseg_conv3x3_bwd_data_bn", (vin, gv, wgt, dx, ldx) + d + (mean, invstd) + tuple(bn_out)),
               "bwd_weight": ("ssdseg_conv3x3_bwd_weight", (vin, ldx, gv, dw) + d)}
        return [out[e] for e in which]

    viewed = ("fwd", "fwd_saved", "fwd_saved_from", "bwd_data_bn", "bwd_weight")
    graded = ("bwd_data", "bwd_data_bn", "bwd_weight")
    everyone = ("fwd", "fwd_saved", "fwd_saved_from", "bwd_weight_saved", "bwd_data", "bwd_data_bn", "bwd_weight")
    calls = []
    for bad in (dict(dims=(0, h, w)), dict(dims=(n, 0, w)), dict(dims=(n, h, -1)), dict(cin=0), dict(cin=cin + 2, ldx=k.ldx + 4), dict(cout=0), dict(cout=cout - 2)):
        calls += calls_of(everyone, **bad)
    calls += calls_of(viewed + ("bwd_data",), ldx=cin - 4)                                      # ldx < cin
    calls += calls_of(viewed, ldx=cin + 2)                                                     # an input (or fused-sums) pitch that is no multiple of 4
    for v in half_views:
        calls += calls_of(viewed, vin=v)
    calls += calls_of(("bwd_data_bn",), vin=dev.view("plain"))                                # the fused sums need the BatchNorm's view
    for v in half_gviews:
        calls += calls_of(graded, gv=v)
    calls += calls_of(("fwd", "fwd_saved", "fwd_saved_from", "bwd_data", "bwd_data_bn"), wgt=None)
    calls += calls_of(("fwd", "fwd_saved", "fwd_saved_from"), y=None)
    calls += calls_of(("bwd_data", "bwd_data_bn"), dx=None)
    calls += calls_of(("bwd_weight", "bwd_weight_saved"), dw=None)
    calls += calls_of(("fwd_saved", "fwd_saved_from", "bwd_weight_saved"), xs=None)
    calls += calls_of(("bwd_weight_saved",), g=None)
    for c_from in (-4, cin, cin + 4, 2):
        calls += calls_of(("fwd_saved_from",), c_from=c_from)
    # a shape ssdseg_conv3x3_saved_floats reports no size for (odd h: no Winograd weight gradient)
    calls += calls_of(("fwd_saved", "fwd_saved_from", "bwd_weight_saved"), dims=(n, h + 1, w))
    calls += calls_of(("bwd_data_bn",), mean=None) + calls_of(("bwd_data_bn",), invstd=None)
    calls += calls_of(("bwd_data_bn",), bn_out=bn_out[:2] + (None, bn_out[3])) + calls_of(("bwd_data_bn",), bn_out=bn_out[:3] + (None,))
    def refused(entry, args):
        def call():
            with pytest.raises(H.SsdsegError, match="invalid argument"):
                ctx.call(entry, *args)
        kernels = launched(ctx, call)
        assert kernels == {}, (entry, kernels)

    for entry, args in calls:
        refused(entry, args)
    # the switches that take the saved pair away refuse its entry points
    for var in ("SSDSEG_CONV3_SAVED", "SSDSEG_CONV3_WGRAD"):
        monkeypatch.setenv(var, "0")
        for entry, args in calls_of(("fwd_saved", "fwd_saved_from", "bwd_weight_saved")):
            refused(entry, args)
        monkeypatch.delenv(var)
    # a NULL ctx is argument 1 of every launching entry point (no ctx: the call goes to the library directly)
    for entry, args in calls_of(everyone):
        conv = [C.c_void_p(a.ptr) if isinstance(a, H.DeviceBuffer) else (C.byref(a) if isinstance(a, (H.ViewStruct, H.GViewStruct)) else a) for a in args]
        kernels = launched(ctx, lambda: conv.append(getattr(ctx.lib, entry)(None, *conv)))
        assert conv[-1] == -1001 and kernels == {}, (entry, conv[-1], kernels)
    for fn in ("ssdseg_conv3x3_parts", "ssdseg_conv3x3_saved_floats"):
        out = C.c_int() if fn.endswith("parts") else C.c_longlong()
        for dims, arg in (((0, h, w, cin, cout), 1), ((n, 0, w, cin, cout), 1), ((n, h, 0, cin, cout), 1), ((n, h, w, 0, cout), 4), ((n, h, w, cin + 2, cout), 4),
                          ((n, h, w, cin, 0), 5), ((n, h, w, cin, cout + 1), 5)):
            assert getattr(ctx.lib, fn)(*dims, C.byref(out)) == -1000 - arg, (fn, dims)
        assert getattr(ctx.lib, fn)(n, h, w, cin, cout, None) == -1006
    ctx.sync()
    for o in (y, dx, dw, table, xs) + bn_out:
        assert untouched(o) == o.size
    # the good calls still run; dgamma / dbeta may be NULL
    r = P.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6)
    dx_, dgamma, dbeta, k1, k0 = bwd_data_bn(ctx, dev, O.ACT_RELU6, O.ACT_RELU6, r"^gemm_rowA_kernel<\d, 1, 1, ")
    assert ratio(dx_, r[0], 0.0) == 0.0 and ratio(dgamma, r[1], 0.0) == 0.0 and ratio(dbeta, r[2], 0.0) == 0.0
    bufs = dev.fresh("dx", "k1out", "k0out")
    ctx.call("ssdseg_conv3x3_bwd_data_bn", vin, gv, wgt, bufs[0], k.ldx, n, h, w, cin, cout, bn_in[0], bn_in[1], None, None, bufs[1], bufs[2])
    assert same_bits(bufs[1].download(), k1) and same_bits(bufs[2].download(), k0) and ratio(bufs[0].download().reshape(n, h, w, cin), r[0], 0.0) == 0.0


# --------------------------------------------------------------------------------------------------------------- coverage
def test_the_suite_reaches_every_kernel_it_is_there_for():
    """every 3x3 kernel symbol tests/test_gpu_conv3_dispatch.py lists as reachable at small shapes is among the launches the timing
    registry recorded, when every lattice case ran in this process"""
    if not RAN >= {nm for nm in P.CASES if nm not in P.SAVED}:
        pytest.skip("not every lattice case ran in this process: the recorded launches are not the suite's")
    assert P.coverage_gaps(RECORDED) == []
