"""The references and cases of tests/_bn_cases.py, vetted on the CPU (oracle and finite differences only).

tests/test_gpu_bn_edges.py compares the BatchNorm-statistics, view and strided helper kernels with these references; this file
shows that the references are right (against oracle.np_ops where it defines the operation, against central differences for the
backward pass) and that the cases reach the edges they are named for.  These are conditions on the inputs and on the references,
not measurements of the code under test.
"""
import numpy as np
import pytest

import _bn_cases as BC
from oracle import np_ops as O

F32 = np.float32
EPS32 = float(F32(BC.EPS))


# ------------------------------------------------------------------------------------------------------------ finalize_ref
def table_of(y, parts):
    """the exact sums of y spread over `parts` rows, as float32"""
    idx = np.arange(y.shape[0]) % parts
    tab = np.zeros((parts, 2, y.shape[1]))
    np.add.at(tab[:, 0], idx, y.astype(np.float64))
    np.add.at(tab[:, 1], idx, y.astype(np.float64) ** 2)
    return tab.astype(F32)


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_finalize_ref_is_the_oracle_for_real_data():
    rng = np.random.default_rng(3)
    m, c = 200, 12
    y = rng.normal(0.5, 2.0, (m, c)).astype(F32)
    p = BC._bn_params(rng, c)
    _, cache = O.bn_train_fwd(y, p["gamma"], p["beta"], eps=EPS32)
    mm_ref, mv_ref = O.bn_moving_update(p["mm0"], p["mv0"], cache, momentum=float(F32(BC.MOMENTUM)))
    ref = BC.finalize_ref(table_of(y, 7), float(m), p["gamma"], p["beta"], BC.EPS, BC.MOMENTUM, p["mm0"], p["mv0"], 1)
    # the table is float32 (2^-24 relative per entry), the oracle's cache as well: 1e-6 holds both
    for name in ("mean", "invstd", "scale"):
        assert rel(cache[name], ref[name]) < 1e-6, name
    assert np.abs(cache["shift"] - ref["shift"]).max() < 1e-6
    assert rel(mm_ref, ref["mm"]) < 1e-6 and rel(mv_ref, ref["mv"]) < 1e-6
    assert (ref["raw_var"] > 0).all() and np.array_equal(ref["var"], ref["raw_var"])
    # inference: the moving statistics as they are
    inf = BC.finalize_ref(None, 0.0, p["gamma"], p["beta"], BC.EPS, BC.MOMENTUM, p["mm0"], p["mv0"], 0)
    s_ref, t_ref = O.bn_infer_affine(p["gamma"], p["beta"], p["mm0"], p["mv0"], eps=EPS32)
    assert rel(s_ref, inf["scale"]) < 1e-6 and np.abs(t_ref - inf["shift"]).max() < 1e-6
    assert np.array_equal(inf["mm"], p["mm0"].astype(np.float64)) and np.array_equal(inf["mean"], inf["mm"])


def test_finalize_ref_at_one_sample():
    case = BC.FINALIZE_CASES["single-sample"]()
    assert case["count"] == 1.0 and case["nparts"] == 1
    ref = BC.finalize_case_ref(case)
    mom = float(F32(BC.MOMENTUM))
    # exact squares: the biased variance is exactly 0 and the moving variance moves towards it -- no Bessel factor (0 / 0)
    assert np.array_equal(ref["raw_var"], np.zeros(case["c"]))
    assert np.array_equal(ref["mv"], case["mv0"].astype(np.float64) * mom)
    assert np.array_equal(ref["invstd"], np.full(case["c"], 1.0 / np.sqrt(EPS32)))
    assert all(np.isfinite(ref[k]).all() for k in ("mean", "invstd", "scale", "shift", "mm", "mv"))
    # the oracle on the one row of samples does the same (it skips the factor at n == 1 as well)
    _, cache = O.bn_train_fwd(case["samples"][None], case["gamma"], case["beta"], eps=EPS32)
    _, mv_ref = O.bn_moving_update(case["mm0"], case["mv0"], cache, momentum=mom)
    assert cache["count"] == 1 and rel(mv_ref, ref["mv"]) < 1e-6 and rel(cache["scale"], ref["scale"]) < 1e-6
    # where it differs from the oracle: it sees the float32 table.  A square that float32 rounds leaves a variance of up to
    # 2^-24 x^2 instead of the oracle's exact 0, and it is clamped when the rounding went down
    x = np.array([1.1, 1.3, 2.7, 0.3], F32)
    tab = np.stack([x, x * x])[None].astype(F32)
    one = BC.finalize_ref(tab, 1.0, np.ones(4, F32), np.zeros(4, F32), BC.EPS, BC.MOMENTUM, np.zeros(4, F32), np.ones(4, F32), 1)
    assert (one["raw_var"] != 0).all() and (one["raw_var"] < 0).any() and (one["raw_var"] > 0).any()
    assert (np.abs(one["raw_var"]) <= BC.U * x.astype(np.float64) ** 2).all()
    assert np.array_equal(one["var"], np.maximum(one["raw_var"], 0))


def test_finalize_ref_clamps_constant_channels():
    case = BC.FINALIZE_CASES["constant-channels"]()
    ref = BC.finalize_case_ref(case)
    const = case["constant"]
    _, cache = O.bn_train_fwd(case["samples"], case["gamma"], case["beta"], eps=EPS32)
    assert np.array_equal(cache["var"][const], np.zeros(const.sum(), F32))      # the oracle: exactly 0
    raw = ref["raw_var"][const]
    assert (raw < 0).any(), "no constant channel folds to a negative variance"
    # 64-term float32 chains: each row sum is within 64 U, so E[x^2] - mean^2 is within 3 * 64 U of 0, relative to x^2
    assert (np.abs(raw) <= 3 * 64 * BC.U * np.asarray(BC.CONSTANTS, np.float64) ** 2).all()
    clamped = const & (ref["raw_var"] <= 0)
    assert np.array_equal(ref["var"][clamped], np.zeros(clamped.sum()))
    assert np.array_equal(ref["invstd"][clamped], np.full(clamped.sum(), 1.0 / np.sqrt(EPS32)))
    assert rel(cache["invstd"][clamped], ref["invstd"][clamped]) < 1e-7
    # the channels with data agree with the oracle as far as float32 row sums allow (64-term chains: 64 * 2^-24)
    assert rel(cache["invstd"][~const], ref["invstd"][~const]) < 1e-5 and rel(cache["mean"][~const], ref["mean"][~const]) < 1e-4
    # 37.5 and its square are short binary fractions: its sums are exact
    assert (raw[np.asarray(BC.CONSTANTS) == 37.5] == 0).all()


# -------------------------------------------------------------------------------------------------------- finalize cases
def test_finalize_tables_have_distinct_rows_and_positive_variance():
    for nparts, c in BC.FINALIZE_PAIRS:
        case = BC.finalize_table(nparts, c)
        t = case["table"]
        assert t.shape == (nparts, 2, c) and t.dtype == F32
        for v in range(2):      # every row's magnitude differs from every other row's, channel by channel
            mag = np.sort(np.abs(t[:, v].astype(np.float64)), axis=0)
            assert (np.diff(mag, axis=0) > 0).all(), (nparts, c, v)
        ref = BC.finalize_case_ref(case)
        assert (ref["raw_var"] > 1.0).all()
        # a row dropped or counted twice moves the mean by far more than 4 ulps
        moved = np.abs(t[:, 0].astype(np.float64)).min(axis=0) / case["count"]
        assert (moved > 1000 * 4 * BC.ULP * np.abs(ref["mean"])).all()


def test_finalize_pairs_cover_every_reduce_template_on_both_sides_of_each_switch():
    rc = {pair: BC.reduce_rc(*pair) for pair in BC.FINALIZE_PAIRS}
    assert set(rc.values()) == {2, 8, 32}
    assert rc[(31, 20)] == 32 and rc[(32, 20)] == 8                 # the 31 / 32 row switch
    assert rc[(255, 24)] == 8 and rc[(256, 24)] == 2                # the 255 / 256 row switch
    assert rc[(2048, 16)] == 2 and rc[(300, 2052)] == 8             # the 2048-channel switch at 256 rows and above
    assert [rc[p] for p in BC.FINALIZE_PAIRS] == [32, 32, 32, 8, 8, 8, 8, 2, 2, 2, 2, 8]
    for want in (2, 8, 32):     # a ragged last block and a row count off the 4-chain stride in every template
        pairs = [p for p in BC.FINALIZE_PAIRS if rc[p] == want]
        assert any(c % want for _, c in pairs), want
        assert any(n % (4 * (256 // want)) for n, _ in pairs), want
    # the special cases: 64 rows x 16 channels, 1 row, inference (always 32)
    assert BC.reduce_rc(64, 16) == 8 and BC.reduce_rc(1, 12) == 32


# ------------------------------------------------------------------------------------------------------------- row cases
def test_row_geometries_reach_the_block_shapes():
    launch = {g: BC.row_launch(g[0], g[1]) for g in BC.ROW_GEOMETRIES}
    assert launch[(1, 4, 4)] == dict(cv=1, bx=1, by=64, gx=1, gy=1)                     # one lane by 64 rows, one row of data
    assert launch[(7, 4, 12)]["by"] == 64                                              # m < blockDim.y
    assert launch[(63, 12, 12)] == dict(cv=3, bx=3, by=64, gx=1, gy=1)
    assert launch[(513, 20, 36)]["gx"] == 2 and launch[(4099, 96, 160)]["gx"] == 25
    assert launch[(300, 1028, 1032)] == dict(cv=257, bx=256, by=2, gx=19, gy=2)         # second grid column: one active lane
    assert launch[(16400, 1024, 1024)]["gx"] == BC.MAX_PARTS == 1024                    # wants 1025 partial rows
    assert max(m * ld * 4 for m, _, ld in BC.ROW_GEOMETRIES) < 65 << 20                 # the largest buffer: 64 MiB
    assert all(ld >= c and ld % 4 == 0 and c % 4 == 0 for _, c, ld in BC.ROW_GEOMETRIES)
    assert sum(ld > c for _, c, ld in BC.ROW_GEOMETRIES) >= 4


@pytest.mark.parametrize("geom", BC.ROW_GEOMETRIES, ids=BC.geometry_id)
def test_row_cases_are_stable_and_barely_nudged(geom):
    case = BC.row_case(*geom)
    assert case["nudged"] < 0.01
    scale, shift = BC.batch_affine(case["y"], case["gamma"], case["beta"])
    z = BC.preact64(case["y"], scale, shift)
    zr = BC.preact64(case["res"], case["rscale"], case["rshift"])
    for t in (z, zr):
        assert BC.boundary_distance(t, O.ACT_RELU6) >= BC.BAND
    if geom[0] >= 63:       # every branch of both activations is taken
        assert (z < 0).any() and ((z > 0) & (z < 6)).any() and (z > 6).any()
    assert len(set(case["pitches"])) == (3 if geom[2] > geom[1] else 1)


def test_boundary_case_expectations_are_the_oracle():
    case = BC.boundary_case()
    y = case["y"]
    for ch in range(8):         # every channel sees every value
        assert sorted(case["index"][:, ch].tolist()) == list(range(8))
    assert (case["g"] != 0).all() and np.array_equal(case["g"], np.round(case["g"]))
    assert y[case["index"] == 3][0] == F32(2.0 ** -140) > 0 and np.signbit(y[case["index"] == 1]).all()
    for act in BC.ACTS:
        assert np.array_equal(O.act_mask(y, act), np.asarray(BC.BOUNDARY_MASKS[act], F32)[case["index"]])
        assert np.array_equal(O.act_fwd(y, act), BC.BOUNDARY_OUTPUTS[act][case["index"]])
    # strict at exactly 0 and exactly 6
    assert BC.BOUNDARY_MASKS[O.ACT_RELU6][2] == 0 and BC.BOUNDARY_MASKS[O.ACT_RELU6][5] == 0 and BC.BOUNDARY_MASKS[O.ACT_RELU][2] == 0


# -------------------------------------------------------------------------------------------------- backward references
@pytest.mark.parametrize("act", BC.ACTS, ids=BC.ACT_NAMES.get)
def test_bn_bwd_ref_matches_finite_differences(act):
    """L = sum w * act(gamma * (y - mean(y)) * invstd(y) + beta), all in float64: dL/dy is the gradient view
    scale * mask * w + k1 * y + k0, dL/dgamma and dL/dbeta are the two sums"""
    m, c, eps = 6, 4, EPS32
    rng = np.random.default_rng(17)
    y = rng.normal(0.5, 1.5, (m, c))
    gamma, beta, w = rng.uniform(1, 3, c), rng.normal(2, 2, c), rng.normal(0, 1, (m, c))

    def stats(t):
        mean = t.mean(axis=0)
        return mean, 1.0 / np.sqrt(t.var(axis=0) + eps)

    def affine(t):
        mean, invstd = stats(t)
        return gamma * invstd, beta - mean * gamma * invstd

    assert BC.stabilise(y, affine) < 0.05
    assert BC.boundary_distance(BC.preact64(y, *affine(y)), O.ACT_RELU6) >= BC.BAND

    def loss(t, gm, bt):
        mean, invstd = stats(t)
        return float((w * O.act_fwd(gm * (t - mean) * invstd + bt, act)).sum())

    def central(f, x, h=1e-6):
        out = np.zeros_like(x)
        for i in np.ndindex(x.shape):
            hi, lo = x.copy(), x.copy()
            hi[i] += h
            lo[i] -= h
            out[i] = (f(hi) - f(lo)) / (2 * h)
        return out

    mean, invstd = stats(y)
    scale, shift = affine(y)
    ref = BC.bn_bwd_ref(w, y, scale, shift, mean, invstd, act, m)
    dy, mask, _ = BC.gview_ref(w, y, scale, shift, ref["k1"], ref["k0"], act)
    tol = 1e-7 * max(1.0, float(np.abs(w).sum()))
    assert np.abs(dy - central(lambda t: loss(t, gamma, beta), y)).max() < tol
    assert np.abs(ref["dgamma"] - central(lambda t: loss(y, t, beta), gamma)).max() < tol
    assert np.abs(ref["dbeta"] - central(lambda t: loss(y, gamma, t), beta)).max() < tol
    if act == O.ACT_ZERO:
        assert not dy.any() and not any(ref[k].any() for k in ("dgamma", "dbeta", "k1", "k0"))
    else:
        assert np.abs(dy).max() > 0.1
    # the same through the oracle's closed form
    cache = dict(mean=mean, invstd=invstd, scale=scale, count=m)
    dy_o, dg_o, db_o = O.bn_train_bwd(w * mask, y, gamma, cache)
    assert np.abs(dy - dy_o).max() < 1e-12 and np.abs(ref["dgamma"] - dg_o).max() < 1e-12 and np.abs(ref["dbeta"] - db_o).max() < 1e-12


def test_bounds_scale_with_the_absolute_sums():
    # chain_bound: the longest chain a thread sums plus the in-block fold, for the geometries in use
    for m, c, _ in BC.ROW_GEOMETRIES:
        launch = BC.row_launch(m, c)
        per_thread = -(-m // (launch["gx"] * launch["by"]))
        assert per_thread <= -(-m // launch["gx"]) and launch["by"] <= BC.MAX_BLOCK_Y
        assert BC.chain_bound(m, launch["gx"]) >= 2 * (per_thread + launch["by"]) * BC.U
    assert BC.chain_bound(16400, 1024) == 2 * (17 + 64) * 2.0 ** -24


@pytest.mark.parametrize("geom", [g for g in BC.ROW_GEOMETRIES if BC.row_launch(g[0], g[1])["gx"] > 1], ids=BC.geometry_id)
def test_a_lost_partial_row_is_outside_the_chain_bound(geom):
    """the sums of squares of one block's rows (block p takes the rows [p * by, (p + 1) * by) of every gx * by) against the bound
    the whole sum is held to: a table row that is never written, or never folded, cannot hide in the tolerance"""
    m, c, _ = geom
    launch = BC.row_launch(m, c)
    gx, by = launch["gx"], launch["by"]
    sq = BC.row_case(*geom)["y"].astype(np.float64) ** 2
    padded = np.zeros((-(-m // (gx * by)) * gx * by, c))
    padded[:m] = sq
    rows = padded.reshape(-1, gx, by, c).sum(axis=(0, 2))
    assert rows.shape == (gx, c) and np.abs(rows.sum(axis=0) - sq.sum(axis=0)).max() < 1e-6 * sq.sum(axis=0).max()
    assert (rows > 5 * BC.chain_bound(m, gx) * sq.sum(axis=0)).all()


def test_axpby_ref_is_exact_arithmetic():
    rng = np.random.default_rng(5)
    s, d = rng.standard_normal((9, 8), F32), rng.standard_normal((9, 8), F32)
    for a, b in BC.AXPBY_COEFFS:
        exact = a * s.astype(np.float64) + b * d.astype(np.float64)
        assert np.array_equal(BC.axpby_ref(a, b, s, d), exact.astype(F32))
    assert np.isfinite(BC.axpby_ref(0.5, 0.0, s, np.full_like(d, np.nan))).all()
