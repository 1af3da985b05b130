"""GPU parity of the BatchNorm-statistics, view and strided helper kernels at their edges (through the C-ABI) vs float64.

ssdseg_bn_finalize, ssdseg_channel_stats, ssdseg_bn_apply, ssdseg_bn_bwd_reduce, ssdseg_gview_materialize, ssdseg_axpby
(csrc/bn.hip) and ssdseg_act_bwd (csrc/shuffle.hip) on the cases of tests/_bn_cases.py: row pitches with a gap, every activation
code, every reduce_parts template (csrc/reduce_parts.h) on both sides of its switch points, count == 1, clamped variances, the
block shapes of row_launch.  tests/test_cpu_bn_cases.py vets the references and the cases.  Every buffer is guarded
(tests/_guard.py): a gap column read yields a NaN, a gap column written is reported, an element left unwritten stays a NaN.
The last test runs the same reduction as column sums (csrc/colsum.hip): a mixed batch of deferred tables against the same
tables folded one launch each.

The bounds are derived, not tuned.  U = 2^-24 is the float32 unit roundoff, ULP = 2^-23 one ulp relative.

  finalize      The kernel folds the float32 table in float64 and rounds every output once; so does finalize_ref, from the same
                table (float64 noise is 2^-53 per operation, 2^-29 of a float32 rounding even after 2048 of them).  One rounding is
                U; allowed: 4 ULP of |reference| for mean, invstd, scale and the moving statistics.  shift = beta - mean * scale is
                a difference, so its rounding is not relative to itself after cancellation but the float64 noise of its terms is:
                allowed 4 ULP of |beta| + |mean * scale|.
  channel_stats A thread sums at most ceil(m / nparts) rows in a float32 chain, the block folds at most 64 such sums in float32,
                the rows of the table are folded in float64 here.  A chain of n terms is within (n - 1) U / (1 - n U) of the sum
                of absolute terms; allowed 2 (ceil(m / nparts) + 64) U sum |x| (and sum x^2 for the squares, which enter through
                a fused multiply-add: one rounding per term as well).
  bn_apply      out = act(fma(s, x, t)) + ract(fma(rs, r, rt)): each term is one rounding of its pre-activation (the clamp moves a
                value towards a representable bound, never away from the float64 clamp by more than that rounding), the sum one
                more: U (|a| + |b|) + U |a + b| <= ULP (|a| + |b|).  Allowed: 2 ULP of |a| + |b|, the magnitude of the result
                before cancellation -- |a + b| alone is not a valid scale when the two views cancel, and without a residual the two
                are the same number.
  bn_bwd_reduce The chain bound above over sum |mask g| for dbeta and over sum |mask g xhat| for dgamma, whose terms also carry 4 ULP
                for xhat = (y - mean) * invstd formed in float32; one final rounding U of each output; k1 = -scale dgamma invstd /
                count and k0 = scale (dgamma invstd mean - dbeta) / count inherit the two errors through these formulas
                (_bn_cases.bn_bwd_bounds).  The reference is fed the device's scale, shift, mean and invstd.
  gview         dy = mask scale g + (k1 y + k0): at most four roundings, each relative to a partial result that is at most
                S = |mask scale g| + |k1 y| + |k0|: 3 U S.  Allowed 3 ULP of S.
  act_bwd, axpby  exact: a product with 0 or 1; coefficients that are powers of two leave one rounding, which float32 NumPy shares.

Run with -s for the largest error / bound ratio of every case (DESIGN.md records them).
"""
import numpy as np
import pytest

import _bn_cases as BC
from oracle import np_ops as O
from _guard import INPUT_WORD, assert_finite_rows, guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
GEOM_ACT = [(g, a) for g in BC.ROW_GEOMETRIES for a in BC.ACTS]


def geom_act_id(v):
    return BC.geometry_id(v) if isinstance(v, tuple) else BC.ACT_NAMES[v]


def report(kernel, case, **ratios):
    """prints and asserts the error / bound ratios of one case"""
    print(f"\nbn-edges {kernel} {case}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, f"{kernel} {case}: {k} is {v:.3g} x its bound"


def ratio(got, ref, bound):
    """largest |got - ref| / bound; where the bound is 0 the result must be exact"""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} elements are not finite"
    err = np.abs(got - ref)
    exact = bound == 0
    assert not err[exact].any(), "an element whose bound is 0 differs"
    return float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0


def finish(ctx, guards):
    ctx.sync()
    guards.check()


def device_affine(ctx, guards, case):
    """channel_stats -> bn_finalize on the device for the case's y (at its first pitch): the scale, shift, mean and invstd the
    other kernels are then given, as device buffers and as the arrays they hold"""
    m, c, ld = case["m"], case["c"], case["pitches"][0]
    y = guards.inp(case["y"], ld=ld)
    nparts = ctx.parts("ssdseg_channel_stats_parts", m, c)
    stats = guards.out((nparts, 2, c))
    ctx.call("ssdseg_channel_stats", y, ld, m, c, stats)
    out = dict(y=y, ld=ld, nparts=nparts)
    bufs = [guards.out(c) for _ in range(4)]
    ctx.call("ssdseg_bn_finalize", stats, nparts, c, float(m), guards.inp(case["gamma"]), guards.inp(case["beta"]), BC.EPS, BC.MOMENTUM,
             None, None, *bufs, 1)
    for name, buf in zip(("mean", "invstd", "scale", "shift"), bufs):
        out[name] = buf
        out[name + "_h"] = buf.download()
        assert np.isfinite(out[name + "_h"]).all(), name
    return out


def unit_affine(guards, c):
    return guards.inp(np.ones(c, F32)), guards.inp(np.zeros(c, F32))


# -------------------------------------------------------------------------------------------------------------- finalize
@pytest.mark.parametrize("name", list(BC.FINALIZE_CASES))
def test_bn_finalize_edges(ctx, guards, name):
    case = BC.FINALIZE_CASES[name]()
    ref = BC.finalize_case_ref(case)
    c, training = case["c"], case["training"]
    table = guards.inp(case["table"]) if training else None
    moving = case["mm0"] is not None
    if not moving:
        mm = mv = None
    elif training:      # updated in place
        mm, mv = guards.out(c).upload(case["mm0"]), guards.out(c).upload(case["mv0"])
    else:               # read only
        mm, mv = guards.inp(case["mm0"]), guards.inp(case["mv0"])
    mean, invstd, scale, shift = (guards.out(c) for _ in range(4))
    ctx.timing(True)
    ctx.timing_reset()
    try:
        ctx.call("ssdseg_bn_finalize", table, case["nparts"], c, case["count"], guards.inp(case["gamma"]), guards.inp(case["beta"]),
                 BC.EPS, BC.MOMENTUM, mm, mv, mean, invstd, scale, shift, training)
        ctx.join()
        launches = {k: r["count"] for k, r in ctx.timing_report().items()}
    finally:
        ctx.timing(False)
    assert launches == {"bn_finalize_kernel": 1}
    got = dict(mean=mean.download(), invstd=invstd.download(), scale=scale.download(), shift=shift.download())
    if moving:
        got.update(mm=mm.download(), mv=mv.download())
    ratios = {k: ratio(got[k], ref[k], 4 * BC.ULP * (ref["shift_mag"] if k == "shift" else np.abs(ref[k]))) for k in got}
    report("bn_finalize", name, **ratios)
    if name == "single-sample":     # the moving variance moves towards the biased variance 0: no 0 / 0 Bessel factor
        assert np.array_equal(got["mv"], (case["mv0"].astype(np.float64) * float(F32(BC.MOMENTUM))).astype(F32))
        assert np.array_equal(got["invstd"], np.full(c, 1.0 / np.sqrt(float(F32(BC.EPS)))).astype(F32))
    if name == "constant-channels":
        clamped = case["constant"] & (ref["raw_var"] <= 0)
        assert (ref["raw_var"] < 0).any()
        assert np.array_equal(got["invstd"][clamped], np.full(int(clamped.sum()), 1.0 / np.sqrt(float(F32(BC.EPS)))).astype(F32))
    finish(ctx, guards)


# --------------------------------------------------------------------------------------------------------- channel_stats
@pytest.mark.parametrize("form", ["pitch", "view"])
@pytest.mark.parametrize("geom", BC.ROW_GEOMETRIES, ids=BC.geometry_id)
def test_channel_stats_edges(ctx, guards, geom, form):
    case = BC.row_case(*geom)
    m, c, ld = geom
    y = case["y"]
    if form == "pitch":
        x = guards.inp(y, ld=ld)
    else:       # a channel slice at the right edge of a wider buffer: the pitch comes with a base pointer offset
        ld = ld if ld > c else c + 4
        wide = np.full((m, ld), INPUT_WORD, np.uint32).view(F32)
        wide[:, ld - c:] = y
        x = guards.inp(wide).view(ld - c, (m, c))
    nparts = ctx.parts("ssdseg_channel_stats_parts", m, c)
    assert nparts == BC.row_launch(m, c)["gx"]
    if m == 16400:
        assert nparts == 1024
    stats = guards.out((nparts, 2, c))
    ctx.call("ssdseg_channel_stats", x, ld, m, c, stats)
    table = stats.download()
    assert_finite_rows(table, "channel stats")
    tot = BC.fold(table)
    y64 = y.astype(np.float64)
    cb = BC.chain_bound(m, nparts)
    report("channel_stats", f"{BC.geometry_id(geom)} {form}", sum=ratio(tot[0], y64.sum(axis=0), cb * np.abs(y64).sum(axis=0)),
           sumsq=ratio(tot[1], (y64 * y64).sum(axis=0), cb * (y64 * y64).sum(axis=0)))
    finish(ctx, guards)


# -------------------------------------------------------------------------------------------------------------- bn_apply
# (in: activation, affine view?; residual: None | "identity" | "affine", its activation)
APPLY_CONFIGS = {
    "none-affine": (O.ACT_NONE, True, None, O.ACT_NONE),
    "none-identity": (O.ACT_NONE, False, None, O.ACT_NONE),
    "relu-identity+identity": (O.ACT_RELU, False, "identity", O.ACT_NONE),
    "relu6-affine+relu-affine": (O.ACT_RELU6, True, "affine", O.ACT_RELU),
    "zero-affine+relu6-affine": (O.ACT_ZERO, True, "affine", O.ACT_RELU6),
    "relu6-identity+none-affine": (O.ACT_RELU6, False, "affine", O.ACT_NONE),
    "relu-affine+zero-identity": (O.ACT_RELU, True, "identity", O.ACT_ZERO),
}


@pytest.mark.parametrize("config", list(APPLY_CONFIGS))
@pytest.mark.parametrize("geom", BC.ROW_GEOMETRIES, ids=BC.geometry_id)
def test_bn_apply_edges(ctx, guards, geom, config):
    from ssdseglib import _hip as H
    case = BC.row_case(*geom)
    m, c = case["m"], case["c"]
    ldx, ldr, ldo = case["pitches"]
    act, affine, residual, ract = APPLY_CONFIGS[config]
    if affine:
        aff = device_affine(ctx, guards, case)
        view, scale, shift = H.view(aff["y"], aff["scale"], aff["shift"], act), aff["scale_h"], aff["shift_h"]
    else:
        view, scale, shift = H.view(guards.inp(case["y"], ld=ldx), act=act), None, None
    rview = rscale = rshift = None
    if residual == "identity":
        rview = H.view(guards.inp(case["res"], ld=ldr), act=ract)
    elif residual == "affine":
        rscale, rshift = case["rscale"], case["rshift"]
        rview = H.view(guards.inp(case["res"], ld=ldr), guards.inp(rscale), guards.inp(rshift), ract)
    out = guards.out((m, c), ld=ldo)
    ctx.call("ssdseg_bn_apply", view, ldx, rview, ldr if rview is not None else 0, out, ldo, m, c)
    ref, mag = BC.bn_apply_ref(case["y"], scale, shift, act, case["res"] if residual else None, rscale, rshift, ract)
    report("bn_apply", f"{BC.geometry_id(geom)} {config}", out=ratio(out.download(), ref, 2 * BC.ULP * mag))
    finish(ctx, guards)


@pytest.mark.parametrize("act", BC.ACTS, ids=BC.ACT_NAMES.get)
def test_bn_apply_boundary_values(ctx, guards, act):
    from ssdseglib import _hip as H
    case = BC.boundary_case()
    want = BC.BOUNDARY_OUTPUTS[act][case["index"]]
    y = guards.inp(case["y"])
    for affine in (unit_affine(guards, 8), (None, None)):
        out = guards.out((8, 8))
        ctx.call("ssdseg_bn_apply", H.view(y, *affine, act), 8, None, 0, out, 8, 8, 8)
        got = out.download()
        assert np.array_equal(got, want), f"values {BC.BOUNDARY_VALUES[np.unique(case['index'][got != want])]} are not clamped exactly"
    finish(ctx, guards)


# --------------------------------------------------------------------------------------------------------- bn_bwd_reduce
def run_bwd_reduce(ctx, guards, case, aff, g, ldg, act, with_sums=True):
    c = case["c"]
    outs = [guards.out(c) if with_sums or i >= 2 else None for i in range(4)]
    ctx.call("ssdseg_bn_bwd_reduce", g, ldg, aff["y"], aff["ld"], case["m"], c, aff["scale"], aff["shift"], aff["mean"], aff["invstd"], act, *outs)
    return {k: (b.download() if b is not None else None) for k, b in zip(("dgamma", "dbeta", "k1", "k0"), outs)}


@pytest.mark.parametrize("geom,act", GEOM_ACT, ids=geom_act_id)
def test_bn_bwd_reduce_edges(ctx, guards, geom, act):
    case = BC.row_case(*geom)
    m, c = case["m"], case["c"]
    ldg = case["pitches"][1]
    aff = device_affine(ctx, guards, case)
    host = [aff[k + "_h"] for k in ("scale", "shift", "mean", "invstd")]
    # the masks of the reference are the kernel's: no float64 pre-activation within half the band of a kink, a float32 one moves 2^-24
    assert BC.boundary_distance(BC.preact64(case["y"], host[0], host[1]), act) > BC.BAND / 2
    got = run_bwd_reduce(ctx, guards, case, aff, guards.inp(case["g"], ld=ldg), ldg, act)
    ref = BC.bn_bwd_ref(case["g"], case["y"], *host, act, m)
    bounds = BC.bn_bwd_bounds(ref, host[0], host[2], host[3], m, m, aff["nparts"])
    if act == O.ACT_ZERO:
        assert all(not got[k].any() for k in got)
    report("bn_bwd_reduce", f"{BC.geometry_id(geom)} {BC.ACT_NAMES[act]}", **{k: ratio(got[k], ref[k], bounds[k]) for k in got})
    finish(ctx, guards)


def test_bn_bwd_reduce_without_sums(ctx, guards):
    """dgamma = dbeta = NULL (the BatchNorm has no trainable parameters to update): the same coefficients bit for bit"""
    case = BC.row_case(513, 20, 36)
    ldg = case["pitches"][1]
    aff = device_affine(ctx, guards, case)
    g = guards.inp(case["g"], ld=ldg)
    full = run_bwd_reduce(ctx, guards, case, aff, g, ldg, O.ACT_RELU6)
    bare = run_bwd_reduce(ctx, guards, case, aff, g, ldg, O.ACT_RELU6, with_sums=False)
    assert bare["dgamma"] is None and bare["dbeta"] is None
    for k in ("k1", "k0"):
        assert np.isfinite(bare[k]).all() and np.array_equal(bare[k].view(np.uint32), full[k].view(np.uint32))
    finish(ctx, guards)


@pytest.mark.parametrize("act", BC.ACTS, ids=BC.ACT_NAMES.get)
def test_bn_bwd_reduce_boundary_values(ctx, guards, act):
    """scale = 1, shift = 0, mean = 0, invstd = 1: dbeta is the exact integer sum of the gradient under the strict mask"""
    case = BC.boundary_case()
    one, zero = unit_affine(guards, 8)
    aff = dict(y=guards.inp(case["y"]), ld=8, scale=one, shift=zero, mean=zero, invstd=one)
    got = run_bwd_reduce(ctx, guards, dict(m=8, c=8), aff, guards.inp(case["g"]), 8, act)
    mask = np.asarray(BC.BOUNDARY_MASKS[act], np.float64)[case["index"]]
    assert np.array_equal(got["dbeta"], (mask * case["g"]).sum(axis=0))
    ref = BC.bn_bwd_ref(case["g"], case["y"], np.ones(8), np.zeros(8), np.zeros(8), np.ones(8), act, 8)
    assert np.array_equal(ref["dbeta"], (mask * case["g"]).sum(axis=0))
    bounds = BC.bn_bwd_bounds(ref, np.ones(8), np.zeros(8), np.ones(8), 8, 8, 1)
    report("bn_bwd_reduce", f"boundary {BC.ACT_NAMES[act]}", **{k: ratio(got[k], ref[k], bounds[k]) for k in got})
    finish(ctx, guards)


# ----------------------------------------------------------------------------------------------------- gview_materialize
@pytest.mark.parametrize("geom,act", GEOM_ACT, ids=geom_act_id)
def test_gview_materialize_edges(ctx, guards, geom, act):
    from ssdseglib import _hip as H
    case = BC.row_case(*geom)
    m, c = case["m"], case["c"]
    aff = device_affine(ctx, guards, case)
    host = [aff[k + "_h"] for k in ("scale", "shift", "mean", "invstd")]
    assert BC.boundary_distance(BC.preact64(case["y"], host[0], host[1]), act) > BC.BAND / 2
    # coefficients that are never zero, whatever the activation of the view: those of the ReLU6 backward pass
    coeff = BC.bn_bwd_ref(case["g"], case["y"], *host, O.ACT_RELU6, m)
    k1, k0 = coeff["k1"].astype(F32), coeff["k0"].astype(F32)
    if m > 1:
        assert k1.any() and k0.any()
    g = guards.out((m, c), ld=aff["ld"]).upload(case["g"])      # in place
    ctx.call("ssdseg_gview_materialize", H.gview(g, aff["y"], aff["scale"], aff["shift"], guards.inp(k1), guards.inp(k0), act), aff["ld"], m, c)
    ref, _, mag = BC.gview_ref(case["g"], case["y"], host[0], host[1], k1, k0, act)
    report("gview_materialize", f"{BC.geometry_id(geom)} {BC.ACT_NAMES[act]}", dy=ratio(g.download(), ref, 3 * BC.ULP * mag))
    finish(ctx, guards)


@pytest.mark.parametrize("act", BC.ACTS, ids=BC.ACT_NAMES.get)
def test_gview_materialize_boundary_values(ctx, guards, act):
    from ssdseglib import _hip as H
    case = BC.boundary_case()
    one, zero = unit_affine(guards, 8)
    g = guards.out((8, 8)).upload(case["g"])
    ctx.call("ssdseg_gview_materialize", H.gview(g, guards.inp(case["y"]), one, zero, zero, zero, act), 8, 8, 8)
    mask = np.asarray(BC.BOUNDARY_MASKS[act], F32)[case["index"]]
    got = g.download()
    wrong = got != mask * case["g"]
    assert not wrong.any(), f"the mask is wrong at the values {BC.BOUNDARY_VALUES[np.unique(case['index'][wrong])]}"
    finish(ctx, guards)


# --------------------------------------------------------------------------------------------------------------- act_bwd
@pytest.mark.parametrize("geom,act", GEOM_ACT, ids=geom_act_id)
def test_act_bwd_edges(ctx, guards, geom, act):
    case = BC.row_case(*geom)
    m, c = case["m"], case["c"]
    ldx, ldg, _ = case["pitches"]
    x = case["y"].copy()
    x.ravel()[::17] = 0.0       # the mask is strict: exact kinks among the data
    x.ravel()[5::23] = 6.0
    g = guards.out((m, c), ld=ldg).upload(case["g"])
    ctx.call("ssdseg_act_bwd", g, ldg, guards.inp(x, ld=ldx), ldx, m, c, act)
    assert np.array_equal(g.download(), case["g"] * O.act_mask(x, act))
    finish(ctx, guards)


@pytest.mark.parametrize("act", BC.ACTS, ids=BC.ACT_NAMES.get)
def test_act_bwd_boundary_values(ctx, guards, act):
    case = BC.boundary_case()
    g = guards.out((8, 8)).upload(case["g"])
    ctx.call("ssdseg_act_bwd", g, 8, guards.inp(case["y"]), 8, 8, 8, act)
    mask = np.asarray(BC.BOUNDARY_MASKS[act], F32)[case["index"]]
    got = g.download()
    wrong = got != mask * case["g"]
    assert not wrong.any(), f"the mask is wrong at the values {BC.BOUNDARY_VALUES[np.unique(case['index'][wrong])]}"
    finish(ctx, guards)


# ----------------------------------------------------------------------------------------------------------------- axpby
@pytest.mark.parametrize("a,b", BC.AXPBY_COEFFS)
@pytest.mark.parametrize("geom", BC.ROW_GEOMETRIES, ids=BC.geometry_id)
def test_axpby_edges(ctx, guards, geom, a, b):
    case = BC.row_case(*geom)
    m, c = case["m"], case["c"]
    lds, ldd, _ = case["pitches"]
    dst = guards.out((m, c), ld=ldd)
    if b != 0:
        dst.upload(case["res"])
    else:       # b == 0 must not read the destination: its body stays poison (NaN) until the call
        assert len(guards.unwritten(dst)) == m * c
    ctx.call("ssdseg_axpby", guards.inp(case["y"], ld=lds), lds, dst, ldd, m, c, a, b)
    got = dst.download()
    assert np.isfinite(got).all()
    assert np.array_equal(got, BC.axpby_ref(a, b, case["y"], case["res"]))
    finish(ctx, guards)


@pytest.mark.parametrize("geom", BC.ROW_GEOMETRIES, ids=BC.geometry_id)
def test_axpby_in_place(ctx, guards, geom):
    """dst == src with (1, 1), as the data-parallel warm-up uses it: every element doubles"""
    case = BC.row_case(*geom)
    m, c, ld = case["m"], case["c"], case["pitches"][0]
    buf = guards.out((m, c), ld=ld).upload(case["y"])
    ctx.call("ssdseg_axpby", buf, ld, buf, ld, m, c, 1.0, 1.0)
    assert np.array_equal(buf.download(), case["y"] + case["y"])
    finish(ctx, guards)


# ------------------------------------------------------------------------------------------------- deferred column sums
def test_mixed_deferred_batch_routes_every_table_to_its_blocks(ctx, guards, monkeypatch):
    """Four ssdseg_dwconv_bwd calls whose slab tables take every route of the column-sum dispatch (_dw_cases.COLSUM_MIX: block shapes
    32, 8, 2, 32 over 3, 9, 72 and 144 blocks), launched one by one and then as ONE colsum_batch_kernel (csrc/colsum.hip): table ->
    block shape -> block range.  Integer lattice, identity views, no dx: every dW is exact, so the two runs and the float64
    reference agree bit for bit.  In the deferred run the first call is made twice into the same dW, first with another g, last of
    all with the right one: the later table wins and its blocks come last."""
    import os
    import _dw_cases as D
    from _edge_helpers import launched
    from ssdseglib import _hip as H
    for v in D.DW_VARS + ("SSDSEG_COLSUM_RC",):
        monkeypatch.delenv(v, raising=False)
    assert not [v for v in D.MARCH_ENV if v in os.environ]
    calls, conv = [], {}
    for shape in D.COLSUM_MIX:
        n, h, w, c = shape
        x, wgt, g, other = D.colsum_mix_case(shape)
        ref, ref_other = (O.dwconv_bwd(x.astype(np.float64), wgt.astype(np.float64), gg.astype(np.float64), 1, 1)[1] for gg in (g, other))
        assert ref.any() and not np.array_equal(ref, ref_other)
        symbol = D.bwd_plan(n, h, w, c, 1, 1, {}, has_dx=False)["symbol"]
        conv[symbol] = conv.get(symbol, 0) + 1
        calls.append(dict(dims=(n, h, w, c, 1, 1, 0), x=guards.inp(x), w=guards.inp(wgt), g=guards.inp(g), other=guards.inp(other),
                          dw=guards.out((3, 3, c)), ref=ref))

    def run(k, g):
        ctx.call("ssdseg_dwconv_bwd", H.view(k["x"]), k["w"], H.gview(k[g]), None, k["dw"], *k["dims"])

    kernels = launched(ctx, lambda: [run(k, "g") for k in calls])
    assert kernels == dict(conv, colsum_kernel=4), kernels
    immediate = [k["dw"].download() for k in calls]
    for k in calls:
        guards.repoison(k["dw"])
    conv[D.bwd_plan(*calls[0]["dims"][:6], {}, has_dx=False)["symbol"]] += 1
    try:
        ctx.colsum_defer(True)
        kernels = launched(ctx, lambda: [run(calls[0], "other")] + [run(k, "g") for k in calls[1:]] + [run(calls[0], "g")])
    finally:
        ctx.colsum_defer(False)
    assert kernels == dict(conv, colsum_batch_kernel=1), kernels
    for k, first in zip(calls, immediate):
        got = k["dw"].download()
        assert np.array_equal(got, first), k["dims"]
        assert np.array_equal(got, k["ref"]) and np.array_equal(first, k["ref"]), k["dims"]
    finish(ctx, guards)
