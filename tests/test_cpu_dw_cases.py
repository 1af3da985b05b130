"""CPU: the cases, the reference and the launch-geometry mirror of tests/_dw_cases.py, vetted without a GPU.

A case is only worth running if it has the property it is named for, whatever its seed draws.  So, on the reference alone:
the mirror reproduces ssdseg_dwconv_parts (the library's host code runs without a device) and the values pinned in
tests/test_cpu_dwconv_parts.py; every named case has the chunk length, chunk count, last-chunk length, strips per block, strip
groups, channel chunks and grid trips it claims; every lattice case evaluates to the same numbers in float32 and in float64 and
keeps every reduction below 2^24 units of its lattice; both thresholds of ReLU6 are hit in both views; and each structural error
a kernel could make -- swapped or shifted pads, a seam row dropped or doubled, a halo column lost between strips, ragged columns
taken as present, a sub-grid shifted or cut, a partial row lost, a non-strict mask, an ignored accumulate, fused sums taken before
the accumulation -- moves the reference by at least one unit of the lattice (normal family: by at least 10 x the bound).

The normal family is shown the same errors through the same generators (seams of a dense and of a dilated case, strip halos, ragged
columns, sub-grid edges, pads, accumulate, the order of the fused sums).  The mirror's kernel symbols, template flags included, are
checked against the table pinned in tests/test_gpu_depthwise_dispatch.py.

Blind by construction, and named here: a pad swap where pt == pl (odd x odd and even x even stride-2 shapes); the mask convention in
the normal family (nothing lies on a threshold), and in lattice cases of fewer than 256 gradient elements, where a draw may leave a
threshold without a non-zero gradient on it; an empty dW row of one image's block in the cases of 2048 and 4096 one-strip images
(their statistics rows are checked for every image, their dW rows are not).
"""
import ctypes as C
import os

import numpy as np
import pytest

import _dw_cases as D
from oracle import np_ops as O

F32 = np.float32
SMALL = [name for name, case in D.CASES.items() if case[7] == "all" and name not in D.ONE_SETTING]
STRIDE2 = [name for name in SMALL if D.CASES[name][4] == 2]
DILATED = [name for name in SMALL if D.CASES[name][5] > 1]


def units(k):
    """lattice units of (y, dx, dW, dbeta, dgamma)"""
    xd, wd = float(k.xd), float(k.wd)
    return 1 / (xd * wd), 1 / (xd * xd * wd), 1 / xd ** 3, 1 / (xd * xd * wd), 1 / (2 * xd ** 3 * wd)


def moved(a, b, unit):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) >= unit


# -------------------------------------------------------------------------------------------------------------- the mirror
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ssdseglib import _hip
    if not os.path.exists(_hip.library_path()):
        g.build()
    return _hip.load_library()


def test_march_switches_are_unset():
    assert not [v for v in D.MARCH_ENV if v in os.environ]


@pytest.mark.parametrize("name", list(D.CASES))
def test_mirror_gives_the_librarys_table_rows(lib, name):
    shape = D.shape_of(name)
    v = C.c_int()
    assert lib.ssdseg_dwconv_parts(*shape, C.byref(v)) == 0
    assert v.value == D.dw_fwd_table_rows(*shape)


def test_mirror_gives_the_pinned_table_rows():
    from test_cpu_dwconv_parts import PARTS
    for shape, rows in PARTS.items():
        assert D.dw_fwd_table_rows(*shape) == rows, shape


def test_mirror_names_the_pinned_instantiations():
    """the kernel symbols the mirror expects, template flags included, against the table recorded in
    tests/test_gpu_depthwise_dispatch.py: every shape, operand form, kernel family and switch of it"""
    import conftest
    import test_gpu_depthwise_dispatch as P
    envs = {f: {v: value for v, value in conftest.KERNEL_FAMILIES[f].items() if v in D.DW_VARS} for f in P.FAMILIES}
    envs.update({name: dict([pair]) for name, pair in P.SWITCHES.items()})
    checked = 0
    for (form, *shape), per_setting in P.EXPECTED.items():
        entry, _, what = form.partition(":")
        for settings, want in per_setting.items():
            conv = [sym for sym in want if sym.startswith("(dw_")]
            assert len(conv) == 1
            for setting in settings.split():
                if entry == "fwd":
                    plan = D.fwd_plan_env(*shape, envs[setting])
                else:
                    plan = D.bwd_plan(*shape, envs[setting], has_dx="nodx" not in what, accumulate="acc1" in what, has_bn=entry == "bwd_bn")
                    assert ("bn_bwd_partial_kernel" in want) == (entry == "bwd_bn" and not plan["fuse"])
                assert plan["symbol"] == conv[0], (form, shape, setting)
                checked += 1
    assert checked > 1000


def test_same_pad_is_the_oracles():
    for size in range(1, 40):
        for s, d in ((1, 1), (2, 1), (1, 2), (1, 3), (1, 6), (1, 12)):
            assert D.same_pad(size, s, d) == O.same_pad(size, 3, s, d)[:2]


# ------------------------------------------------------------------------------------------- the geometry a case is named for
ROW_CLAIMS = {1: (1, 1, 1), 2: (2, 1, 2), 3: (3, 1, 3), 8: (8, 1, 8), 9: (5, 2, 4), 13: (7, 2, 6), 17: (5, 4, 2), 43: (6, 8, 1)}


def marches(name):
    """the forward's and the backward's march geometry of a case under the default switches"""
    shape = D.shape_of(name)
    f, b = D.fwd_plan_env(*shape, {}), D.bwd_plan(*shape, {})
    assert f["family"] == "march" and b["family"] == ("march" if shape[4] == 1 else "march2")
    return f["launch"], b["launch"]


@pytest.mark.parametrize("rows", list(ROW_CLAIMS))
@pytest.mark.parametrize("suffix", ["", "-s2"])
def test_row_chunk_cases(rows, suffix):
    for l in marches(f"rows{rows}{suffix}"):
        assert (l["rows"], l["chunks"], l["last"]) == ROW_CLAIMS[rows]
        assert l["rows"] * (l["chunks"] - 1) + l["last"] == rows


def test_row_chunk_cases_cover_the_loop_forms():
    """chunk lengths 1, 2 (below the prefetch depth), odd and even lengths against the two-row unrolled loop and the three-stage forward"""
    lengths = set()
    for rows, (chunk, chunks, last) in ROW_CLAIMS.items():
        lengths.update({chunk, last})
    assert {1, 2, 3} <= lengths and {l % 2 for l in lengths} == {0, 1} and {l % 3 for l in lengths} == {0, 1, 2}


@pytest.mark.parametrize("name", ["halved-once", "halved-once-s2"])
def test_halving_stops_midway(name):
    for l in marches(name):
        assert l["halvings"] == 1 and l["rows"] > 8 and l["chunks"] >= 2 and l["waves"] >= D.MARCH_MIN_WAVES


@pytest.mark.parametrize("name", ["one-chunk", "one-chunk-s2", "one-chunk-wide", "one-chunk-wide-s2"])
def test_no_halving_one_long_chunk(name):
    for l in marches(name):
        assert l["halvings"] == 0 and l["chunks"] == 1 and l["rows"] > 8 and l["waves"] >= D.MARCH_MIN_WAVES
    if "wide" in name:
        assert marches(name)[0]["sgroups"] == 86 and marches(name)[0]["cchunks"] == 6 and marches(name)[0]["waves"] == 4128


def test_column_cases():
    strips = {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 7: 2, 8: 2, 9: 3}
    for w, want in strips.items():
        f, b = marches(f"cols{w}")
        assert f["wstrips"] == b["wstrips"] == want
        assert D.bwd_plan(*D.shape_of(f"cols{w}"), {})["wfull"] == (w % 4 == 0)
    assert {w % 4 for w in strips} == {0, 1, 2, 3}               # a last strip of one, two, three and four columns
    for name in ("strips-wasted", "strips-wasted-s2"):
        for l in marches(name):
            assert l["spb"] == 3 and l["sgroups"] == 2 and l["wasted"] == 1 and l["wstrips"] == 5


def test_stride2_pad_pairs():
    for wo, ws in ((1, (1, 2)), (3, (5, 6))):
        pairs = set()
        for h in (5, 6):
            for w in ws:
                g = D.dw_geom(*D.shape_of(f"pads-{h}x{w}-s2"))
                assert g["wo"] == wo
                pairs.add((g["pt"], g["pl"]))
        assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_channel_cases():
    want = {4: (4, 1), 60: (60, 1), 128: (64, 2), 144: (144, 1), 260: (130, 2), 1284: (214, 6)}
    for c, (cb, cchunks) in want.items():
        for name in (f"chan{c}", f"chan{c}-s2"):
            for l in marches(name):
                assert (l["cb"], l["cchunks"]) == (cb, cchunks)
    assert 130 % 64 != 0 and 214 % 64 != 0          # ragged last lane group of a chunk


def subgrids(h, w, d):
    return [((h - a + d - 1) // d, (w - b + d - 1) // d) for a in range(d) for b in range(d)]


def test_dilation_cases():
    assert len(set(subgrids(5, 7, 2))) == 4                                        # four sub-grids of different sizes
    f, b = marches("dil2-h19")
    assert {r for r, _ in subgrids(19, 6, 2)} == {10, 9} and f["rows"] == b["rows"] == 5 and f["chunks"] == 2     # 9 rows end inside chunk 2
    assert sum(1 for r, c in subgrids(4, 5, 12) if r > 0 and c > 0) == 20 and len(subgrids(4, 5, 12)) == 144      # empty sub-grids
    assert len(set(subgrids(7, 5, 3))) > 1 and len(set(subgrids(13, 13, 6))) > 1
    for name in DILATED:
        shape = D.shape_of(name)
        assert D.fwd_plan_env(*shape, D.SETTINGS["gather"])["family"] == "gather"
        assert D.bwd_plan(*shape, D.SETTINGS["gather"])["family"] == "gather"
        assert D.bwd_plan(*shape, {})["family"] == "march"


def test_grid_stride_cases():
    for name, (setting,) in D.ONE_SETTING.items():
        if not name.startswith("trips"):
            continue
        shape, env = D.shape_of(name), D.SETTINGS[setting]
        f, b = D.fwd_plan_env(*shape, env), D.bwd_plan(*shape, env)
        assert b["family"] == setting and b["launch"]["trips"] >= 2, name
        assert f["launch"]["trips"] >= 2, name
    assert D.dw_geom(*D.shape_of("trips-reg"))["ntiles"] > 65536 and D.dw_geom(*D.shape_of("trips-gather"))["ntiles"] > 65536
    assert D.lds_launch(D.dw_geom(*D.shape_of("trips-lds")))["tiles"] > 1024
    spread = D.lds_launch(D.dw_geom(*D.shape_of("trips-lds-spread")))
    assert spread["spread"] and spread["tiles"] > spread["grid_x"] and spread["cgroups"] * 32 > D.shape_of("trips-lds-spread")[3]


def test_families_of_the_settings():
    for name in SMALL:
        shape = D.shape_of(name)
        n, h, w, c, s, d = shape
        if d > 1:
            continue
        assert D.fwd_plan_env(*shape, D.SETTINGS["lds"])["family"] == "lds"
        assert D.bwd_plan(*shape, D.SETTINGS["lds"])["family"] == ("lds" if s == 1 else "reg")
        assert D.bwd_plan(*shape, D.SETTINGS["reg"])["family"] == "reg"
        assert D.fwd_plan_env(*shape, D.SETTINGS["depth1"])["depth2"] is False
        assert D.fwd_plan_env(*shape, {})["depth2"] is (s == 1)
        assert D.bwd_plan(*shape, D.SETTINGS["march"])["family"] == D.bwd_plan(*shape, {})["family"]


def test_colsum_mix_takes_every_route_of_the_column_sum_dispatch():
    """the four shapes of the mixed deferred batch (tests/test_gpu_bn_edges.py): few rows, exactly at the 32-row switch, exactly at
    the 256-row switch, the wide route -- three block shapes, four block ranges of different lengths"""
    import _bn_cases as BC
    assert [D.bwd_plan(*shape, 1, 1, {})["rows"] for shape in D.COLSUM_MIX] == [8, 32, 256, 8]
    assert [9 * shape[3] for shape in D.COLSUM_MIX] == [72, 72, 144, 4608]
    for shape, (rows, rc) in D.COLSUM_MIX.items():
        assert D.bwd_plan(*shape, 1, 1, {})["rows"] == rows and D.colsum_rc(rows, 9 * shape[3]) == rc, shape
    assert [rc for _, rc in D.COLSUM_MIX.values()] == [32, 8, 2, 32]
    # each value sits on its switch: one row fewer, or one column fewer than the wide route, gives another block shape
    assert D.colsum_rc(31, 72) == 32 and D.colsum_rc(255, 144) == 8 and D.colsum_rc(256, 2048) == 8
    assert D.colsum_rc(8, 4608) == D.colsum_rc(256, 4608) == 32 and D.colsum_rc(256, 4095) == BC.reduce_rc(256, 4095) == 8
    blocks = [D.cdiv(9 * shape[3], rc) for shape, (_, rc) in D.COLSUM_MIX.items()]
    assert blocks == [3, 9, 72, 144]


def test_forms_cover_the_views():
    fwd_views = {v for v, _ in D.FWD_FORMS}
    assert fwd_views == {"plain"} | set(D.ACTS) and {s for _, s in D.FWD_FORMS} == {True, False}
    assert {v for v, *_ in D.BWD_FORMS} == {"plain"} | set(D.ACTS)
    assert {g for _, g, *_ in D.BWD_FORMS} == {"identity"} | set(D.ACTS)
    assert {(dx, acc) for _, _, dx, acc in D.BWD_FORMS} == {(True, 0), (True, 1), (False, 0), (False, 1)}
    assert {acc for *_, acc in D.BN_FORMS} == {0, 1}


# ------------------------------------------------------------------------------------------------------ the lattice is exact
@pytest.mark.parametrize("name", list(D.CASES))
def test_lattice_float32_equals_float64_and_stays_in_budget(name):
    k = D.lattice_case(name)
    for q, v in D.budget(k).items():
        assert v < D.EXACT, (q, v / D.EXACT)
    fwd_forms, bwd_forms, bn_forms = D.forms_of(name)
    for view in {v for v, _ in fwd_forms}:
        for a, b in zip(D.ref_fwd(k, view), D.ref_fwd(k, view, F32)):
            assert b.dtype == F32 and np.array_equal(a, b.astype(np.float64)), ("fwd", view)
    for view, gview, has_dx, acc in bwd_forms:
        for a, b in zip(D.ref_bwd(k, view, gview, acc), D.ref_bwd(k, view, gview, acc, F32)):
            assert b.dtype == F32 and np.array_equal(a, b.astype(np.float64)), ("bwd", view, gview, acc)
    for view, gview, acc in bn_forms:
        for a, b in zip(D.ref_bn(k, view, gview, acc)[:4], D.ref_bn(k, view, gview, acc, F32)[:4]):
            assert b.dtype == F32 and np.array_equal(a, b.astype(np.float64)), ("bn", view, gview, acc)


@pytest.mark.parametrize("name", list(D.CASES))
def test_lattice_inputs_are_on_their_lattice(name):
    k = D.lattice_case(name)
    for f in ("x", "g", "yraw", "base", "shift", "gshift", "k1", "k0", "mean"):
        v = getattr(k, f).astype(np.float64) * k.xd
        assert np.array_equal(v, np.round(v)), f
    v = k.w.astype(np.float64) * k.wd
    assert np.array_equal(v, np.round(v))
    for f in ("scale", "gscale", "invstd"):
        m, _ = np.frexp(np.abs(getattr(k, f)))
        assert (m == 0.5).all(), f                       # powers of two


@pytest.mark.parametrize("name", SMALL)
def test_thresholds_are_hit_and_the_strict_mask_matters(name):
    k = D.lattice_case(name)
    uy, udx, udw, udb, udg = units(k)
    zin = k.x.astype(np.float64) * k.scale + k.shift
    zg = k.yraw.astype(np.float64) * k.gscale + k.gshift
    if k.g.size >= 256:
        for z in (zin, zg):
            assert (z == 0).sum() > 0 and (z == 6).sum() > 0
    for act in (O.ACT_RELU, O.ACT_RELU6):
        dx, dw = D.ref_bwd(k, O.ACT_RELU6, act, 0)
        dx2, dw2 = D.ref_bwd(k, O.ACT_RELU6, act, 0, gview_nonstrict=True)
        if k.g.size >= 256:
            assert moved(dx, dx2, udx) and moved(dw, dw2, udw)
        r, r2 = D.ref_bn(k, act, O.ACT_RELU6, 1), D.ref_bn(k, act, O.ACT_RELU6, 1, view_nonstrict=True)
        if k.g.size >= 256:
            assert moved(r[3], r2[3], udb) and moved(r[2], r2[2], udg)


def test_sparse_cases_hit_the_lower_threshold():
    for name, case in D.CASES.items():
        if case[6] == "sparse":
            k = D.lattice_case(name)
            assert (k.x == 0).mean() > 0.5 and ((k.x.astype(np.float64) * k.scale) == 6).sum() > 0


# ------------------------------------------------------------------------------- structural errors move the reference
@pytest.mark.parametrize("name", STRIDE2)
def test_pad_errors_move_y(name):
    k = D.lattice_case(name)
    n, h, w, c, s, d = k.shape
    uy = units(k)[0]
    g = D.dw_geom(*k.shape)
    a, _ = D.in_view(k, O.ACT_RELU6)
    w64 = k.w.astype(np.float64)
    y = D.ref_fwd(k, O.ACT_RELU6)[0]
    assert np.array_equal(D.conv_fwd_pads(a, w64, s, d, g["pt"], g["pl"]), y)          # the helper itself
    if g["pt"] != g["pl"]:
        assert moved(D.conv_fwd_pads(a, w64, s, d, g["pl"], g["pt"]), y, uy)
    for dpt, dpl in ((1, 0), (0, 1), (-1, 0), (0, -1)):
        pt, pl = g["pt"] + dpt, g["pl"] + dpl
        if pt >= 0 and pl >= 0:
            assert moved(D.conv_fwd_pads(a, w64, s, d, pt, pl), y, uy), (dpt, dpl)


def test_pad_swap_is_seen_somewhere():
    assert sum(1 for name in STRIDE2 if D.dw_geom(*D.shape_of(name))["pt"] != D.dw_geom(*D.shape_of(name))["pl"]) >= 4


# Each generator below yields (label, kind, wrong, right): what a kernel with one structural error would give against the reference,
# full-size arrays of the output `kind` ("y" | "sum" | "dx" | "dW").  The lattice tests ask for a difference of one unit of the
# kind's lattice, the normal family's for 10 x the kind's bound somewhere.
R6 = O.ACT_RELU6


def operands(k):
    a, _ = D.in_view(k, R6)
    return a, k.w.astype(np.float64), D.g_view(k, R6)


def seam_rows(k):
    """the image rows on both sides of every chunk seam of the default march (dilated: of every sub-grid, whose row r is image row
    ga + r d)"""
    n, h, w, c, s, d = k.shape
    l = D.fwd_plan_env(*k.shape, {})["launch"]
    rows = []
    for seam in range(l["rows"], D.cdiv(k.ho, d), l["rows"]):
        rows += [ga + sub * d for sub in (seam - 1, seam) for ga in range(d) if ga + sub * d < k.ho]
    return rows


def seam_errors(k):
    """a seam row dropped from (or, with the sign turned, counted twice in) the statistics, dW and the dy that reaches dx"""
    n, h, w, c, s, d = k.shape
    a, wgt, dy = operands(k)
    ysum, dw_rows = D.row_terms(k, R6, R6)
    dx, dw = O.dwconv_bwd(a, wgt, dy, s, d)
    for r in seam_rows(k):
        yield f"row {r}", "sum", ysum.sum(axis=0) - ysum[r], ysum.sum(axis=0)
        yield f"row {r}", "dW", dw - dw_rows[r], dw
        cut = dy.copy()
        cut[:, r] = 0
        yield f"row {r}", "dx", O.dwconv_bwd(a, wgt, cut, s, d)[0], dx


def halo_errors(k):
    """the dy column next to a strip lost to the strip's dx, and the strip's first window column lost to its y"""
    n, h, w, c, s, d = k.shape
    a, wgt, dy = operands(k)
    dx = O.dwconv_bwd(a, wgt, dy, s, d)[0]
    y = O.dwconv_fwd(a, wgt, s, d)
    strip = D.bwd_plan(*k.shape, {})["launch"]["strip"]
    for b in range(strip, k.wo, strip):             # first output column of a strip; b - 1 is its left halo
        for col in ((b - 1, b) if s == 1 else (b - 1,)):      # (stride 2: a strip's dy window has a left halo only)
            cut = dy.copy()
            cut[:, :, col] = 0
            edge = b if s == 1 else b * s - D.dw_geom(*k.shape)["pl"]         # first input column the strip owns
            side = slice(edge, None) if col == b - 1 else slice(0, edge)
            wrong = dx.copy()
            wrong[:, :, side] = O.dwconv_bwd(a, wgt, cut, s, d)[0][:, :, side]
            yield f"strip at {b}, dy column {col}", "dx", wrong, dx
        cut = a.copy()
        cut[:, :, b * s - D.dw_geom(*k.shape)["pl"]] = 0
        wrong = y.copy()
        wrong[:, :, b:] = O.dwconv_fwd(cut, wgt, s, d)[:, :, b:]
        yield f"strip at {b}, first window column", "y", wrong, y


def ragged_errors(k):
    """a kernel that took the missing columns of the last strip as present would read what follows in memory: the next row"""
    a, wgt, _ = operands(k)
    nxt = np.roll(a.reshape(a.shape[0] * a.shape[1], a.shape[2], -1), -1, axis=0).reshape(a.shape)[:, :, :1]
    yield "column w", "y", O.dwconv_fwd(np.concatenate([a, nxt], axis=2), wgt, 1, 1)[:, :, :a.shape[2]], O.dwconv_fwd(a, wgt, 1, 1)


def subgrid_errors(k):
    n, h, w, c, s, d = k.shape
    a, wgt, dy = operands(k)
    y = O.dwconv_fwd(a, wgt, s, d)
    dx = O.dwconv_bwd(a, wgt, dy, s, d)[0]
    # size off by one: the last row / column of a sub-grid is one of the last d rows / columns of the image
    for kind, full in (("y", y), ("dx", dx)):
        for r in range(max(h - d, 0), h):
            cut = full.copy()
            cut[:, r] = 0
            yield f"row {r} cut", kind, cut, full
        for q in range(max(w - d, 0), w):
            cut = full.copy()
            cut[:, :, q] = 0
            yield f"column {q} cut", kind, cut, full
    # origin off by one: a sub-grid computed from its neighbour's pixels; and the dilation ignored
    if h > 1:
        yield "origin row", "y", O.dwconv_fwd(np.roll(a, 1, axis=1), wgt, s, d), y
    yield "origin column", "y", O.dwconv_fwd(np.roll(a, 1, axis=2), wgt, s, d), y
    yield "dilation 1", "y", O.dwconv_fwd(a, wgt, s, 1), y


def has_seams(name):
    return D.fwd_plan_env(*D.shape_of(name), {})["launch"]["chunks"] > 1


def has_strips(name):
    return D.CASES[name][5] == 1 and D.bwd_plan(*D.shape_of(name), {})["launch"]["wstrips"] >= 2


def is_ragged(name):
    n, h, w, c, s, d = D.shape_of(name)
    return s == 1 and d == 1 and w % 4 != 0 and h > 1


MULTI_CHUNK = [name for name in SMALL if has_seams(name)]
HALO = ["cols5", "cols7", "cols8", "cols9", "strips-wasted", "strips-wasted-s2", "chan144", "chan260"]
RAGGED = [name for name in SMALL if is_ragged(name)]
ERRORS = [(seam_errors, name) for name in MULTI_CHUNK] + [(halo_errors, name) for name in HALO] + \
         [(ragged_errors, name) for name in RAGGED] + [(subgrid_errors, name) for name in DILATED]


def test_error_lists_reach_the_cases_they_should():
    assert "dil2-h19" in MULTI_CHUNK and {"rows9", "rows13", "rows17", "rows43", "rows9-s2", "rows43-s2"} <= set(MULTI_CHUNK)
    assert all(has_strips(name) for name in HALO) and len(RAGGED) >= 10 and len(DILATED) == 5
    assert seam_rows(D.lattice_case("dil2-h19")) == [8, 9, 10, 11] and seam_rows(D.lattice_case("rows17")) == [4, 5, 9, 10, 14, 15]


@pytest.mark.parametrize("errors,name", ERRORS, ids=[f"{e.__name__}-{name}" for e, name in ERRORS])
def test_structural_errors_move_the_lattice_reference(errors, name):
    """every seam of every multi-chunk case, every strip boundary, the ragged last strip, every sub-grid edge"""
    k = D.lattice_case(name)
    uy, udx, udw, _, _ = units(k)
    unit = {"y": uy, "sum": uy, "dx": udx, "dW": udw}
    count = 0
    for label, kind, wrong, right in errors(k):
        assert moved(wrong, right, unit[kind]), (label, kind)
        count += 1
    assert count


NOT_DILATED = [name for name in SMALL if D.CASES[name][5] == 1]


@pytest.mark.parametrize("name", NOT_DILATED)
def test_no_partial_row_is_empty(name):
    """every block of the default marches that has work writes a statistics row that is not zero, and a dW row that is not either"""
    k = D.lattice_case(name)
    n, h, w, c, s, d = k.shape
    l = D.fwd_plan_env(*k.shape, {})["launch"]          # (the backward marches over the same chunks and strip groups of dy)
    a, wgt, dy = operands(k)
    y = O.dwconv_fwd(a, wgt, s, d)
    cols = l["spb"] * l["strip"] * (s if s == 1 else 1)
    for rc in range(l["chunks"]):
        for sg in range(l["sgroups"]):
            rows, span = slice(rc * l["rows"], (rc + 1) * l["rows"]), slice(sg * cols, (sg + 1) * cols)
            part = y[:, rows, span]
            assert part.size and (np.abs(part).reshape(n, -1).max(axis=1) >= units(k)[0]).all(), (rc, sg)
            # (blind: the cases of 2048 and 4096 one-strip images, where a sparse draw may leave one image's few dW terms at zero)
            for img in range(n if n <= 2 else 0):
                only = np.zeros_like(dy)
                only[img, rows, span] = dy[img, rows, span]
                assert np.abs(O.dwconv_bwd(a, wgt, only, s, d)[1]).max() >= units(k)[2], (rc, sg, img)


@pytest.mark.parametrize("name", SMALL)
def test_accumulate_and_the_order_of_the_fused_sums_matter(name):
    k = D.lattice_case(name)
    _, udx, _, udb, udg = units(k)
    assert moved(D.ref_bwd(k, O.ACT_RELU6, O.ACT_RELU6, 1)[0], D.ref_bwd(k, O.ACT_RELU6, O.ACT_RELU6, 0)[0], udx)
    if k.g.size >= 256:
        r, r2 = D.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6, 1), D.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6, 1, sums_before_accumulate=True)
        assert moved(r[3], r2[3], udb) and moved(r[2], r2[2], udg)
    dw_zero = D.ref_bwd(k, O.ACT_ZERO, O.ACT_RELU6, 0)
    assert not dw_zero[1].any() and np.array_equal(dw_zero[0], D.ref_bwd(k, O.ACT_RELU6, O.ACT_RELU6, 0)[0])


# ---------------------------------------------------------------------------------------------------------- normal family
@pytest.mark.parametrize("name", D.NORMAL_CASES)
def test_normal_cases_keep_off_the_thresholds(name):
    k = D.normal_case(name)
    assert k.nudged_x < 1e-4 and k.nudged_y < 1e-4
    for v, s, t in ((k.x, k.scale, k.shift), (k.yraw, k.gscale, k.gshift)):
        z = v.astype(np.float64) * s + t
        assert np.minimum(np.abs(z), np.abs(z - 6)).min() >= D.BAND
        assert np.abs(z).max() * D.U < D.BAND / 10            # a rounding of z cannot cross the band


@pytest.mark.parametrize("name", D.NORMAL_CASES)
def test_structural_errors_exceed_ten_bounds_in_the_normal_family(name):
    k = D.normal_case(name)
    n, h, w, c, s, d = k.shape
    f, b = D.fwd_plan_env(*k.shape, {}), D.bwd_plan(*k.shape, {}, True, True, True)
    bound = D.normal_bounds(k, O.ACT_RELU6, O.ACT_RELU6, 1, f, b)
    g = D.dw_geom(*k.shape)
    a, _ = D.in_view(k, O.ACT_RELU6)
    w64 = k.w.astype(np.float64)
    y = D.ref_fwd(k, O.ACT_RELU6)[0]

    def far(got, ref, bnd):
        return (np.abs(got - ref) >= 10 * np.broadcast_to(bnd, ref.shape)).any()

    if s == 2:
        if g["pt"] != g["pl"]:
            assert far(D.conv_fwd_pads(a, w64, s, d, g["pl"], g["pt"]), y, bound["y"])
        assert far(D.conv_fwd_pads(a, w64, s, d, g["pt"] + 1, g["pl"]), y, bound["y"])
        assert far(D.conv_fwd_pads(a, w64, s, d, g["pt"], g["pl"] + 1), y, bound["y"])
    r = D.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6, 1)
    assert far(D.ref_bwd(k, O.ACT_RELU6, O.ACT_RELU6, 0)[0], r[0], bound["dx"])                   # accumulate ignored
    r2 = D.ref_bn(k, O.ACT_RELU6, O.ACT_RELU6, 1, sums_before_accumulate=True)
    assert far(r2[3], r[3], bound["dbeta"]) and far(r2[2], r[2], bound["dgamma"])
    # seams, strip halos, ragged columns and sub-grid edges: the generators of the lattice tests, here against the bounds of the
    # overwriting form
    b0 = D.normal_bounds(k, O.ACT_RELU6, O.ACT_RELU6, 0, f, D.bwd_plan(*k.shape, {}, True, False, True))
    for errors, applies in ((seam_errors, has_seams(name)), (halo_errors, has_strips(name)), (ragged_errors, is_ragged(name)),
                            (subgrid_errors, d > 1)):
        if applies:
            for label, kind, wrong, right in errors(k):
                assert far(wrong, right, b0[kind]), (errors.__name__, label, kind)


def test_normal_cases_reach_every_structural_error():
    names = D.NORMAL_CASES
    assert any(has_seams(n) and D.CASES[n][5] == 1 for n in names) and any(has_seams(n) and D.CASES[n][5] > 1 for n in names)
    assert any(has_strips(n) for n in names) and any(is_ragged(n) for n in names) and any(D.CASES[n][5] > 1 for n in names)
    assert any(D.CASES[n][4] == 2 and D.dw_geom(*D.shape_of(n))["pt"] != D.dw_geom(*D.shape_of(n))["pl"] for n in names)
