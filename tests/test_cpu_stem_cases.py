"""The reference, the cases and the mirror of tests/_stem_cases.py, vetted without a GPU: the float64 reference against torch's conv2d
with autograd in float64 and against the tap-by-tap form the structural errors are built on; every lattice case on its lattice, below
2^24 in every budgeted reduction under every rescale pair it runs, the same numbers in float32 and float64, both ReLU6 thresholds hit in
the gradient view; the mirror against the library's own host functions (ssdseg_stem_conv_parts, ssdseg_stem_direct_eligible,
ssdseg_stem_direct_blocks: they run without a device); every named case with the property it is named for; every structural error a
kernel could make moving the reference by a unit of the lattice or more (by 10 x the bound or more in the normal family), and the cases
that are blind to one by construction named as such; the same for the max-pool's data, ties and errors."""
import ctypes as C
import os

import numpy as np
import pytest

import _stem_cases as P
import _pw_cases as PW
from oracle import np_ops as O

F32 = np.float32
CU_COUNTS = (256, 304, 64)
FWD_CASES = [nm for nm, c in P.CASES.items() if c["fwd"]]
WGRAD_CASES = [nm for nm, c in P.CASES.items() if c["wgrad"]]
SMALL = 3000          # output pixels up to which a case is put through every structural error (the larger ones share their code paths)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ssdseglib import _hip
    if not os.path.exists(_hip.library_path()):
        g.build()
    lib = _hip.load_library()
    lib.ssdseg_stem_direct_eligible.restype, lib.ssdseg_stem_direct_eligible.argtypes = C.c_bool, [C.c_int]
    lib.ssdseg_stem_direct_blocks.restype, lib.ssdseg_stem_direct_blocks.argtypes = C.c_int, [C.c_int, C.c_int]
    return lib


def pairs_of(name):
    return [P.PAIRS[i] for i in P.CASES[name]["pairs"]]


def moved(wrong, ref, unit):
    return np.abs(wrong - ref).max() >= unit


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name,family", [("inst-6", "lattice"), ("pad-3x4", "normal"), ("pad-4x3", "lattice"), ("gemm-3img", "normal"), ("wg-m65-c24", "normal")])
def test_reference_agrees_with_torch_autograd_in_float64(name, family):
    import torch
    import torch.nn.functional as TF
    k = P.lattice_case(name) if family == "lattice" else P.normal_case(name)
    n, h, w, cout = k.shape
    pair = P.PAIRS[1] if family == "lattice" else P.NORMAL_PAIR
    (_, pt, pb), (_, pl, pr) = O.same_pad(h, 3, 2), O.same_pad(w, 3, 2)
    assert (pt, pl) == k.geo[2:]
    for gview in ("identity", O.ACT_RELU6):
        a = torch.tensor(P.rescaled(k, pair).transpose(0, 3, 1, 2).copy())
        wt = torch.tensor(k.w.astype(np.float64).transpose(3, 2, 0, 1).copy(), requires_grad=True)
        b = torch.tensor(k.b.astype(np.float64), requires_grad=True)
        y = TF.conv2d(TF.pad(a, (pl, pr, pt, pb)), wt, b, stride=2)
        y.backward(torch.tensor(P.g_view(k, gview).transpose(0, 3, 1, 2).copy()))
        y_ref = P.ref_fwd(k, pair, True)
        assert np.abs(y.detach().numpy().transpose(0, 2, 3, 1) - y_ref).max() <= 1e-12 * max(np.abs(y_ref).max(), 1.0)
        dw_ref, db_ref = P.ref_bwd(k, pair, gview)
        assert np.abs(wt.grad.numpy().transpose(2, 3, 1, 0) - dw_ref).max() <= 1e-12 * max(np.abs(dw_ref).max(), 1.0)
        assert np.abs(b.grad.numpy() - db_ref).max() <= 1e-12 * max(np.abs(db_ref).max(), 1.0)
        # the tap-by-tap forms (the structural errors below are errors OF them) are the reference when nothing is wrong
        assert np.abs(P.by_taps(k, pair, True) - y_ref).max() <= 1e-12 * max(np.abs(y_ref).max(), 1.0)
        assert np.abs(P.dw_wrong(k, pair, gview) - dw_ref).max() <= 1e-12 * max(np.abs(dw_ref).max(), 1.0)


# ------------------------------------------------------------------------------------------------------- lattice: budgets
@pytest.mark.parametrize("name", list(P.CASES))
def test_lattice_case_is_exact_and_not_degenerate(name):
    """no case leaves the exact family: mode_of raises where no lattice fits; the budgets hold under every pair the case runs"""
    k = P.lattice_case(name)
    n, h, w, cout = k.shape
    xmax, wtop, _, _ = P.LATTICE[k.mode]
    assert np.array_equal(k.x, np.round(k.x)) and k.x.min() >= 0 and k.x.max() == xmax <= 255
    for a, den in ((k.w, 8), (k.b, 8), (k.g, 4), (k.yraw, 4), (k.gshift, 4), (k.k1, 4), (k.k0, 4)):
        assert np.array_equal(a * den, np.round(a * den))
    assert np.abs(k.w).max() <= 1 and np.abs(k.b).max() <= 1
    assert np.array_equal(np.abs(k.gscale), 2.0 ** np.round(np.log2(np.abs(k.gscale))))
    for pair in pairs_of(name):
        s, o = pair
        assert s == 2.0 ** round(np.log2(s)) and o * 2 == round(o * 2)
        b = P.budget(k, pair)
        assert max(b[q] for q in P.MUST_HOLD) < P.EXACT, (pair, b)
        # the same numbers in float32 and float64: the bound is 0
        for bias in (False, True):
            y = P.ref_fwd(k, pair, bias)
            assert np.array_equal(y.astype(F32).astype(np.float64), y)
        assert np.array_equal(P.ref_fwd(k, pair, True, F32).astype(np.float64), P.ref_fwd(k, pair, True))
        for gview in (("identity", O.ACT_RELU6) if P.m_of(name) < 65000 else (O.ACT_RELU6,)):
            for got, ref in zip(P.ref_bwd(k, pair, gview, F32), P.ref_bwd(k, pair, gview)):
                assert np.array_equal(got.astype(np.float64), ref) and np.array_equal(ref.astype(F32).astype(np.float64), ref)
        y = P.ref_fwd(k, pair)
        assert y[:, :, -1].any() and y[:, -1].any() and y[-1].any() and y[..., -1].any(), "the last row, column, image or channel is all zero"
    # every tap of the weight gradient matters where the image has it
    live = np.outer([h > 1, True, h > 2], [w > 1, True, w > 2])          # (two pixels: pt = 0, the third tap is the bottom pad)
    dw = P.ref_bwd(k, pairs_of(name)[0], "identity")[0]
    assert np.array_equal(dw.any(axis=(2, 3)), live), (dw.any(axis=(2, 3)), live)


@pytest.mark.parametrize("name", WGRAD_CASES)
def test_both_relu6_thresholds_are_hit_in_the_gradient_view(name):
    k = P.lattice_case(name)
    z = k.yraw.astype(np.float64) * k.gscale + k.gshift
    need = 0 if z.size < 64 else (1 if z.size < 512 else 2)        # (a one-pixel case has too few values to promise a hit)
    assert (z == 0).sum() >= need and (z == 6).sum() >= need, (name, int((z == 0).sum()), int((z == 6).sum()))
    if need:
        loose = ((z >= 0) & (z <= 6)).astype(np.float64)
        assert not np.array_equal(loose, O.act_mask(z, O.ACT_RELU6))


def test_sum_of_squares_is_exact_in_one_case_of_each_form_at_least():
    """where the sum of y^2 stays below 2^24 units of the squared lattice the GPU file demands the fold of the table exactly; elsewhere
    it bounds it"""
    exact = {}
    for name in FWD_CASES:
        if "stats" in P.CASES[name]["variants"] and P.m_of(name) < SMALL:
            k = P.lattice_case(name)
            if any(P.budget(k, pair)["sumsq"] < P.EXACT for pair in pairs_of(name)):
                for form in P.CASES[name]["forms"]:
                    exact.setdefault("direct" if P.takes_direct(P.FORM_ENV[form], *k.shape) else "gemm", name)
    assert set(exact) == {"direct", "gemm"}, exact


# ---------------------------------------------------------------------------------------------- the mirror and the library
def test_mirror_gives_the_librarys_geometry(lib):
    shapes = [c["shape"] for c in P.CASES.values()] + [(2, 480, 640, 32), (32, 480, 640, 24), (9, 480, 64, 32), (3, 33, 47, 40), (1, 4097, 3, 8),
                                                       (5, 2000, 2000, 16), (1, 1, 300000, 64), (7, 129, 255, 100)]
    v = C.c_int()
    for s in shapes:
        n, h, w, cout = s
        assert lib.ssdseg_stem_conv_parts(*s, C.byref(v)) == 0 and v.value == P.table_rows(*s), s
        assert lib.ssdseg_stem_direct_blocks(n, h) == P.direct_blocks(n, h)
        for env in P.FORM_ENV.values():
            assert P.launch_rows(env, *s) <= v.value
        (ho, pt, _), (wo, pl, _) = O.same_pad(h, 3, 2), O.same_pad(w, 3, 2)
        assert P.same_geometry(h, w) == (ho, wo, pt, pl)
    for cout in range(-4, 140):
        assert bool(lib.ssdseg_stem_direct_eligible(cout)) == P.direct_eligible(cout), cout
    for bad, arg in (((0, 4, 4, 8), 1), ((1, 0, 4, 8), 1), ((1, 4, 0, 8), 1), ((1, 4, 4, 6), 4), ((1, 4, 4, 0), 4)):
        assert lib.ssdseg_stem_conv_parts(*bad, C.byref(v)) == -1000 - arg
    assert lib.ssdseg_stem_conv_parts(1, 4, 4, 8, None) == -1005
    assert [P.same_geometry(s, s)[2] for s in (1, 2, 3, 4, 5)] == [1, 0, 1, 0, 1]


# ------------------------------------------------------------------------------------------------------ the named properties
def test_instantiation_cases():
    """all sixteen templates on two different images; idle lanes for Q not a multiple of 4; four spare threads at QP = 12"""
    for q in range(1, 17):
        n, h, w, cout = P.shape_of(f"inst-{q}")
        assert (n, h, w, cout) == (2, 5, 7, 4 * q) and P.takes_direct({}, n, h, w, cout) and not P.takes_direct(P.FORM_ENV["gemm"], n, h, w, cout)
        assert P.fwd_kernel("direct", n, h, w, cout) == r"^stem_fwd_direct_kernel<%d>$" % q
        assert set(P.CASES[f"inst-{q}"]["variants"]) == {"stats", "bias", "none"} and P.CASES[f"inst-{q}"]["pairs"] == P.ALL_PAIRS
        k = P.lattice_case(f"inst-{q}")
        assert not np.array_equal(k.x[0], k.x[1])
    assert [P.qp_of(q) for q in range(1, 17)] == [4] * 4 + [8] * 4 + [12] * 4 + [16] * 4
    assert sorted({P.ppb_of(q) for q in range(1, 17)}) == [16, 21, 32, 64]
    assert [4 * q for q in range(1, 17) if P.qp_of(q) != q] == [4, 8, 12, 20, 24, 28, 36, 40, 44, 52, 56, 60]
    assert [256 - P.ppb_of(q) * P.qp_of(q) for q in (4, 8, 12, 16)] == [0, 0, 4, 0]


def test_pad_pair_cases():
    seen, valid_counts = set(), set()
    for h in (1, 2, 3, 4):
        for w in (1, 2, 3, 4):
            name = f"pad-{h}x{w}"
            assert P.shape_of(name) == (1, h, w, 8) and P.CASES[name]["forms"] == ("direct", "gemm") and P.CASES[name]["pairs"] == P.ALL_PAIRS
            k = P.lattice_case(name)
            _, ok, _ = P.gather(k, rows=3)
            seen.add(k.geo[2:])
            valid_counts.update(int(c) for c in ok.sum(axis=0).ravel())
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)} and {1, 2, 4, 6, 9} <= valid_counts
    k = P.lattice_case("pad-1x1")
    assert P.gather(k, rows=3)[1].sum() == 1                                  # one pixel with eight padded taps
    _, ok, _ = P.gather(P.lattice_case("pad-4x4"), rows=3)
    assert ok[:, 0, 0, 0].all() and not ok[6:, 0, -1, 0].any() and not ok[2::3, 0, 0, -1].any()      # even: no top / left pad, bottom / right pad
    _, ok, _ = P.gather(P.lattice_case("pad-3x3"), rows=3)
    assert not ok[:3, 0, 0, 0].any() and not ok[0::3, 0, 0, 0].any() and not ok[6:, 0, -1, -1].any() and not ok[2::3, 0, -1, -1].any()


def test_pixels_per_trip_cases():
    assert sorted({ppb for ppb, _ in P.PPT.values()}) == [16, 21, 32, 64] and len(P.PPT) == 20
    for name, (ppb, wo) in P.PPT.items():
        n, h, w, cout = P.shape_of(name)
        assert P.ppb_of(cout // 4) == ppb and P.same_geometry(h, w)[:2] == (1, wo) and P.takes_direct({}, n, h, w, cout) and w in (2 * wo - 1, 2 * wo)
    for ppb in (16, 21, 32, 64):
        assert sorted(wo - ppb for p, wo in P.PPT.values() if p == ppb) == [-1, 0, 1, ppb, ppb + 1]
    assert max(P.shape_of(nm)[2] for nm in P.PPT) == 257 and P.shape_of("ppt-16-129")[2] == 257
    # the table's tail in the direct form: one direct row, two GEMM rows
    assert P.direct_blocks(1, 2) == 1 and P.table_rows(*P.shape_of("ppt-16-129")) == 2


def test_row_walk_and_table_cases():
    for name in ("rows-2050-8", "rows-2050-24"):
        n, h, w, cout = P.shape_of(name)
        assert n * P.same_geometry(h, w)[0] == 2050 and P.direct_blocks(n, h) == P.MAX_BLOCKS and P.takes_direct({}, n, h, w, cout)
    assert P.qp_of(24 // 4) != 24 // 4
    s = P.shape_of("stats-40x40")
    assert (P.direct_blocks(s[0], s[1]), P.gemm_rows(*s), P.table_rows(*s)) == (20, 4, 20)
    s = P.shape_of("stats-3x3-64")
    assert (P.direct_blocks(s[0], s[1]), P.gemm_rows(*s), P.table_rows(*s)) == (4, 1, 4) and P.CASES["stats-3x3-64"]["forms"][0] == "gemm"
    for cout in (68, 100):
        s = P.shape_of(f"fallback-{cout}")
        assert not P.direct_eligible(cout) and not P.takes_direct({}, *s) and P.fwd_kernel("direct", *s).startswith(r"^gemm_rowA_kernel<1, 0, 2")
    assert not P.direct_eligible(6) and not P.direct_eligible(0)


def test_implicit_gemm_cases():
    assert [P.m_of(f"gemm-rows{m}") for m in (1, 127, 128, 129)] == [1, 127, 128, 129]
    assert [P.gemm_rows(*P.shape_of(f"gemm-rows{m}")) for m in (1, 127, 128, 129)] == [1, 1, 1, 2]
    n, h, w, cout = P.shape_of("gemm-3img")
    ho, wo = P.same_geometry(h, w)[:2]
    assert n == 3 and ho * wo == 42 and n * ho * wo < P.BM
    # below 512 blocks rowA_wn keeps 32-wide column tiles: the small shapes run one to six of them; the wider tiles need 65,536 rows
    assert [P.cdiv(c, 32 * PW.rowA_wn(70, c, {})) for c in (4, 12, 36, 68, 100, 164)] == [1, 1, 2, 3, 4, 6]
    for cout, wn in P.GEMM_WN.items():
        assert PW.rowA_wn(P.m_of(f"gemm-wn-c{cout}"), cout, {}) == wn and P.m_of(f"gemm-wn-c{cout}") < PW.ROWA_OCC_ROWS
    for name in FWD_CASES:
        if "gemm" in P.CASES[name]["forms"]:
            assert "stats" in P.CASES[name]["variants"]
    s = P.shape_of(P.BIG)
    assert P.m_of(P.BIG) == 263169 >= PW.ROWA_OCC_ROWS and P.gemm_walk(*s) == 3 > 1 and P.gemm_rows(*s) == 686
    # the smallest square whose blocks walk more than one row tile
    side = next(sd for sd in range(2, 1100, 2) if P.gemm_walk(1, sd, sd, 4) > 1)
    assert side == s[1] == s[2], side
    # it stays in the exact family (sum y included), on the narrowest lattice
    assert P.mode_of(P.BIG) == "tiny"


def test_weight_gradient_cases():
    """the split rule at three CU counts; the named edges at 256"""
    for cus in CU_COUNTS:
        for name in WGRAD_CASES:
            p = P.wgrad_plan(P.m_of(name), P.shape_of(name)[3], cus)
            assert (p["splits"] - 1) * p["sps"] < p["steps"] <= p["splits"] * p["sps"] and 0 < p["last_rows"] <= p["rows_per_split"], (name, cus, p)
            assert p["splits"] == 1 or p["sps"] >= 3
            assert 1 <= p["wn"] <= 3
    assert sorted(P.WG_M) == [1, 63, 64, 65, 257, 513] and P.smallest_m(2) == 257 and P.smallest_m(3) == 513
    for m, nhw in P.WG_M.items():
        for cout in P.WG_COUT:
            assert P.m_of(f"wg-m{m}-c{cout}") == m and P.smallest_m(2, cout) == 257 and P.smallest_m(3, cout) == 513
            p = P.wgrad_plan(m, cout)
            assert (p["steps"], p["splits"]) == {1: (1, 1), 63: (1, 1), 64: (1, 1), 65: (2, 1), 257: (5, 2), 513: (9, 3)}[m]
            assert p["wn"] == 1 and p["jtiles"] == P.cdiv(cout, 32)
    assert P.wgrad_plan(257, 4)["last_rows"] == 65 and P.wgrad_plan(513, 4)["last_rows"] == 129
    assert P.WG_M[513][0] == 3                                   # the three-split case holds three images
    for cout, wn in P.WG_WIDE.items():
        p = P.wgrad_plan(P.m_of(f"wg-wide-c{cout}"), cout)
        assert p["wn"] == wn and p["splits"] > 1 and p["last_rows"] < p["rows_per_split"]
    assert [P.wgrad_plan(131044, c)["jtiles"] for c in P.WG_WIDE] == [1, 2]
    # the smallest such M: one row fewer than 2,045 steps and the chip is not full, wn stays 1
    assert P.wgrad_plan(2044 * 64, 64)["wn"] == 1 and P.wgrad_plan(2044 * 64 + 1, 64)["wn"] == 2
    for name in WGRAD_CASES:
        assert all(P.PAIRS[i][1] != 0 for i in P.CASES[name]["pairs"])            # a padded tap counted as `offset` shows


# ------------------------------------------------------------------------------------------------- structural errors: forward
def _fwd_errors(k, pair, unit_or_bound, normal):
    """each structural error of the forward moves y by a lattice unit (by 10 x the bound) somewhere -> the names of the errors this
    case is blind to by construction"""
    n, h, w, cout = k.shape
    ho, wo, pt, pl = k.geo
    s, o = pair
    ref = P.by_taps(k, pair, True)          # (== ref_fwd: test_reference_agrees_with_torch_autograd_in_float64; the same order of sums as the wrong forms)
    blind = set()

    def shows(wrong):
        d = np.abs(wrong - ref)
        return bool((d >= 10 * unit_or_bound).any()) if normal else bool(d.max() >= unit_or_bound)

    def check(label, wrong, visible):
        if visible:
            assert shows(wrong), (k.name, pair, label)
        else:
            assert np.array_equal(wrong, ref), (k.name, pair, label, "is not blind")
            blind.add(label)

    _, ok, _ = P.gather(k, rows=4)
    check("pads-swapped", P.by_taps(k, pair, True, pt=pl, pl=pt), pt != pl)
    check("pt+1", P.by_taps(k, pair, True, pt=pt + 1), True)
    check("pl+1", P.by_taps(k, pair, True, pl=pl + 1), True)
    for tap in range(9):
        check(f"offset-kept-{tap}", P.by_taps(k, pair, True, keep_offset=tap), o != 0 and not ok[tap].all())
        check(f"offset-dropped-{tap}", P.by_taps(k, pair, True, drop_offset=tap), o != 0 and ok[tap].any())
    nb = P.by_taps(k, pair, True, neighbour=True)
    check("neighbour", nb, not np.array_equal(nb, ref))
    if n > 1:
        assert "neighbour" not in blind, "a tap from the neighbouring image is in bounds and wrong"
    check("k26-dropped", P.by_taps(k, pair, True, drop_k=26), ok[8].any() and bool((P.gather(k, rows=3)[0][8][..., 2] * s + o)[ok[8]].any()))
    check("k27-taken", P.by_taps(k, pair, True, extra_k=True), ok[9].any() and bool((P.gather(k)[0][9][..., 0] * s + o)[ok[9]].any()))
    for label in ("last-column", "last-row"):
        check(label, _without(ref, label), True)
    return blind


def _without(ref, label):
    wrong = ref.copy()
    if label == "last-column":
        wrong[:, :, -1] = 0
    else:
        wrong[:, -1] = 0
    return wrong


@pytest.mark.parametrize("name", [nm for nm in FWD_CASES if P.m_of(nm) < SMALL])
def test_forward_structural_errors_move_the_lattice_reference(name):
    k = P.lattice_case(name)
    for i in P.CASES[name]["pairs"]:
        pair = P.PAIRS[i]
        blind = _fwd_errors(k, pair, pair[0] / 8, False)
        offsets = {b for b in blind if b.startswith("offset-")}
        if pair[1] == 0:
            # the (1, 0) and (2^-7, 0) pairs fold nothing but the scale: blind to every offset error by construction
            assert len(offsets) == 18
        else:
            _, ok, _ = P.gather(k, rows=3)
            assert offsets == {f"offset-kept-{t}" for t in range(9) if ok[t].all()} | {f"offset-dropped-{t}" for t in range(9) if not ok[t].any()}
        # a pad swap where pt == pl changes nothing
        assert ("pads-swapped" in blind) == (k.geo[2] == k.geo[3])


def test_what_the_pad_pair_cases_see_together():
    """over the sixteen pad cases every offset error at every tap is seen by some case under the pairs that fold an offset"""
    seen = set()
    for h in (1, 2, 3, 4):
        for w in (1, 2, 3, 4):
            k = P.lattice_case(f"pad-{h}x{w}")
            blind = _fwd_errors(k, P.PAIRS[0], P.PAIRS[0][0] / 8, False)
            seen |= {f"offset-{kind}-{t}" for kind in ("kept", "dropped") for t in range(9)} - blind
    assert len(seen) == 17 and "offset-kept-4" not in seen           # (the centre tap is never padded)


def test_second_pixel_and_idle_lane_errors_move_the_statistics():
    for name, (ppb, wo) in P.PPT.items():
        k = P.lattice_case(name)
        for pair in pairs_of(name):
            y = P.ref_fwd(k, pair)
            second = y[:, :, ppb:2 * ppb]
            if wo <= ppb:
                assert second.size == 0                           # blind by construction: no thread has a second pixel
            else:
                # skipped: the pixels keep their poison and the sums lose them; doubled: the sums gain them
                assert second.any() and np.abs(second.sum(axis=(0, 1, 2))).max() >= pair[0] / 8
            if wo > 2 * ppb:
                assert y[:, :, 2 * ppb:].any()                    # the second trip of the ox0 loop
    for q in range(1, 17):
        k = P.lattice_case(f"inst-{q}")
        for pair in pairs_of(f"inst-{q}"):
            s = P.ref_fwd(k, pair).sum(axis=(0, 1, 2))
            if P.qp_of(q) != q:
                # an idle lane works on the last quad's weights: its value in the sums moves one of these four columns
                assert np.abs(s[-4:]).max() >= pair[0] / 8


@pytest.mark.parametrize("name", [nm for nm in P.NORMAL_CASES if P.CASES[nm]["fwd"]])
def test_forward_structural_errors_are_10_bounds_in_the_normal_family(name):
    k = P.normal_case(name)
    bound = np.maximum(P.fwd_bound(k, P.NORMAL_PAIR, True, True), P.fwd_bound(k, P.NORMAL_PAIR, False, True))
    assert (bound > 0).all() and bound.max() < 1e-4
    blind = _fwd_errors(k, P.NORMAL_PAIR, bound, True)
    assert not {b for b in blind if b.startswith("offset-kept")} - {f"offset-kept-{t}" for t in range(9) if P.gather(k, rows=3)[1][t].all()}


# ----------------------------------------------------------------------------------------- structural errors: weight gradient
@pytest.mark.parametrize("name", [nm for nm in WGRAD_CASES if P.m_of(nm) < SMALL])
def test_weight_gradient_structural_errors_move_the_lattice_reference(name):
    k = P.lattice_case(name)
    m, cout = P.m_of(name), k.shape[3]
    p = P.wgrad_plan(m, cout)
    for pair in pairs_of(name):
        unit = pair[0] / 16
        for gview in ("identity", O.ACT_RELU6):
            ref = P.ref_bwd(k, pair, gview)[0]
            assert np.array_equal(P.dw_wrong(k, pair, gview), ref)
            _, ok, _ = P.gather(k, rows=3)
            if not ok.all():
                assert moved(P.dw_wrong(k, pair, gview, padded_as_offset=True), ref, unit), (pair, gview, "padded-as-offset")
            if p["splits"] > 1:
                assert moved(P.dw_wrong(k, pair, gview, rows=m - p["last_rows"]), ref, unit), (pair, gview, "last-split")
            # the K = 27 tail: the last reduction row is not zero
            if ok[8].any():
                assert ref[2, 2, 2].any()


@pytest.mark.parametrize("name", [nm for nm in P.NORMAL_CASES if P.CASES[nm]["wgrad"]])
def test_weight_gradient_structural_errors_are_10_bounds_in_the_normal_family(name):
    k = P.normal_case(name)
    m, cout = P.m_of(name), k.shape[3]
    p = P.wgrad_plan(m, cout)
    for gview in ("identity", O.ACT_RELU6):
        ref = P.ref_bwd(k, P.NORMAL_PAIR, gview)[0]
        bound = P.bwd_bounds(k, P.NORMAL_PAIR, gview)[0]
        assert (np.abs(P.dw_wrong(k, P.NORMAL_PAIR, gview) - ref) <= 1e-9 * bound.max() + 1e-12).all()
        assert (np.abs(P.dw_wrong(k, P.NORMAL_PAIR, gview, padded_as_offset=True) - ref) >= 10 * bound).any()
        if p["splits"] > 1:
            assert (np.abs(P.dw_wrong(k, P.NORMAL_PAIR, gview, rows=m - p["last_rows"]) - ref) >= 10 * bound).any()


def test_normal_bounds_are_positive_and_small():
    for name in P.NORMAL_CASES:
        k = P.normal_case(name)
        z = k.yraw.astype(np.float64) * k.gscale + k.gshift
        assert np.minimum(np.abs(z), np.abs(z - 6)).min() >= P.BAND * 0.99
        y = P.ref_fwd(k, P.NORMAL_PAIR, True)
        for direct in (True, False):
            b = P.fwd_bound(k, P.NORMAL_PAIR, direct, True)
            assert (b > 0).all() and b.max() < 1e-4 * max(np.abs(y).max(), 1.0)
        for gview in ("identity", O.ACT_RELU6):
            dw_b, db_b = P.bwd_bounds(k, P.NORMAL_PAIR, gview)
            dw, db = P.ref_bwd(k, P.NORMAL_PAIR, gview)
            assert (dw_b >= 0).all() and dw_b.max() > 0 and dw_b.max() < 1e-2 * max(np.abs(dw).max(), 1.0) and (db_b > 0).all() and db_b.max() < 1e-2 * max(np.abs(db).max(), 1.0)
    assert (P.DIRECT_C1, P.DIRECT_C2) == (17, 3)
    assert len(P.NORMAL_CASES) >= 12 and P.NORMAL_PAIR[0] == float(F32(1 / 127.5))


# ------------------------------------------------------------------------------------------------------------ the max-pool
def _pool(k, view):
    a = P.pool_in(k, view)
    wins = P.pool_windows(a)
    ties = wins == wins.max(axis=0)
    first, last = ties.argmax(axis=0), 8 - ties[::-1].argmax(axis=0)
    return a, wins, ties, first, last


@pytest.mark.parametrize("shape", P.POOL_SHAPES, ids=lambda s: "x".join(str(d) for d in s))
def test_pool_cases_and_their_structural_errors(shape):
    k = P.pool_case(shape)
    n, h, w, c = shape
    g = k.g.astype(np.float64)
    assert np.array_equal(k.x * 4, np.round(k.x * 4)) and np.array_equal(k.g * 4, np.round(k.g * 4)) and k.g.all()
    assert np.array_equal(k.x[0], k.x[-1]) and np.array_equal(k.g[0], k.g[-1])
    for view in P.POOL_VIEWS:
        a, wins, ties, first, last = _pool(k, view)
        assert np.array_equal(a.astype(F32).astype(np.float64), a)
        dx = O.maxpool3x3s2_bwd(a, g)
        assert np.array_equal(wins.max(axis=0), O.maxpool3x3s2_fwd(a)) and np.array_equal(P.pool_bwd_by(a, g, P.one_hot(first)), dx)
        assert np.array_equal(dx.sum(axis=(0, 1, 2)), g.sum(axis=(0, 1, 2)))
        tied = ties.sum(axis=0) > 1
        if view != "plain" and a.size >= 100:
            # a third or more of the activations clamp to exactly 0, and under ReLU6 to exactly 6: a tie is the rule
            if a.size >= 1000:          # (the 100-value shapes scatter around the same fractions)
                assert (a == 0).mean() >= 1 / 3 and (view != O.ACT_RELU6 or ((a == 6).mean() >= 1 / 3 and tied.mean() > 0.5))
            assert tied.any()                                     # (under ReLU only an all-clamped window ties: test_pool_special_cases)
        if tied.any():
            # last maximum in place of first (>= in place of >); a window's gradient given to two cells
            assert np.abs(P.pool_bwd_by(a, g, P.one_hot(last)) - dx).max() >= 0.25
            assert np.abs(P.pool_bwd_by(a, g, ties.astype(np.float64)).sum(axis=(0, 1, 2)) - g.sum(axis=(0, 1, 2))).max() >= 0.25
        else:
            assert a.size < 100 or view == "plain"               # blind: one cell per window, or no two equal maxima in these few windows
        # a padded cell winning: padding that compares as 0
        padded_wins = np.where(np.isfinite(wins), wins, 0.0).max(axis=0)
        if view == "plain" and h * w >= 30:
            assert np.abs(padded_wins - wins.max(axis=0)).max() >= 0.25
        elif view != "plain":
            assert np.array_equal(padded_wins, wins.max(axis=0))      # blind in the value (nothing is below 0) -- the gradient shows it:
            lost = np.where(np.isfinite(wins), wins, 0.0)
            first_p = (lost == lost.max(axis=0)).argmax(axis=0)
            if (first_p != first).any():
                assert np.abs(P.pool_bwd_by(a, g, P.one_hot(first_p) * np.isfinite(wins)).sum(axis=(0, 1, 2)) - g.sum(axis=(0, 1, 2))).max() >= 0.25


def test_pool_shapes_cover_every_window_and_overlap():
    valid, cover = set(), set()
    for h in (1, 2, 3, 4, 5):
        for w in (1, 2, 3, 4, 5):
            assert (2, h, w, 4) in P.POOL_SHAPES
            k = P.pool_case((2, h, w, 4))
            wins = P.pool_windows(k.x.astype(np.float64))
            valid.update(int(v) for v in np.isfinite(wins).sum(axis=0).ravel())
            cover.update(int(v) for v in P.pool_bwd_by(k.x, np.ones(wins.shape[1:]), np.isfinite(wins).astype(np.float64)).ravel())
    assert valid == {1, 2, 3, 4, 6, 9} and cover == {1, 2, 4}          # (3: a one-pixel-wide image)
    assert {(P.same_geometry(h, w)[2:]) for h in (4, 5) for w in (4, 5)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert P.POOL_SHAPES[-3:] == [(2, 7, 9, 24), (1, 8, 6, 116), (3, 6, 5, 232)]


def test_pool_special_cases():
    k = P.pool_case(P.POOL_SPECIAL["all-negative"], "all-negative")
    z = k.x.astype(np.float64) * k.scale + k.shift
    a, wins, ties, first, last = _pool(k, O.ACT_RELU)
    assert (z < 0).all() and not a.any()
    assert np.array_equal(ties, np.isfinite(wins)) and sorted(set(ties.sum(axis=0).ravel())) == [4, 6, 9]
    # the first VALID tap is not tap 0 at a top or left border (h = w = 5: pt = pl = 1)
    assert set(first[:, 0, 0].ravel()) == {4} and set(first[:, 0, 1:].ravel()) == {3} and set(first[:, 1:, 0].ravel()) == {1} and set(first[:, 1:, 1:].ravel()) == {0}
    k = P.pool_case(P.POOL_SPECIAL["signed-zeros"], "signed-zeros")
    a, wins, ties, first, last = _pool(k, "plain")
    assert (k.x <= 0).all()
    both = (ties & (wins == 0) & np.signbit(wins)).any(axis=0) & (ties & (wins == 0) & ~np.signbit(wins)).any(axis=0)
    assert both.mean() > 0.25                                     # -0.0 and +0.0 tie for the maximum of a window
    # the first of them wins whatever its sign: a kernel that orders -0.0 below +0.0 routes the gradient elsewhere
    ordered = np.where(wins == 0, np.where(np.signbit(wins), -1e-9, 1e-9), wins)
    assert ((ordered == ordered.max(axis=0)).argmax(axis=0) != first).any()
