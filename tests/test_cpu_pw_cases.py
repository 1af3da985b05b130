"""CPU: the cases, the reference and the host-rule mirror of tests/_pw_cases.py, vetted without a GPU.

A case is only worth running if it has the property it is named for, whatever its seed draws.  So, on the reference alone: the
mirror reproduces ssdseg_pwconv_parts and ssdseg_pwconv_wt_floats (the library's host code runs without a device) on both sides of
every threshold, and the kernel symbols and launch counts pinned in tests/test_gpu_pointwise_dispatch.py, every row, form and family
of that table; every named case has the tile counts, ragged remainders, WN, NT, splits and tiles per wave it claims; every lattice
case evaluates to the same numbers in float32 (in a scrambled order) and in float64 and keeps every reduction below 2^24 units of its
lattice; both thresholds of ReLU6 are hit in both views; and each structural error a kernel could make -- the last row, the last
reduction vector or the last column tile dropped, the row past a split counted, `>=` for `>` at a threshold, a gap column read, the
residual skipped -- moves the reference by at least one unit of the lattice.

Blind by construction, and named here: the mask convention in the normal family and in the sparse cases (no shifts: only the
threshold 0, and `0 * g` hides it for ReLU), and in cases of fewer than 400 elements, where a draw may leave a threshold empty.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _pw_cases as P
from oracle import np_ops as O

F32 = np.float32
SMALL = [name for name in P.CASES if P.CASES[name]["forms"] == "all"]
LARGE = [name for name in P.CASES if P.CASES[name]["forms"] == "large"]


def geom(name, setting, entry, **kw):
    m, k, n = P.shape_of(name)
    ld, env = P.pitches(name), P.SETTINGS[setting]
    if entry == "fwd":
        return P.plan_fwd(m, k, n, ld["x"], env, **kw)
    if entry == "bwd_data":
        return P.plan_bwd_data(m, k, n, ld["y"], env, kw.pop("coef", True), kw.pop("adds", False), **kw)
    if entry == "bwd_weight":
        return P.wgrad_plan(m, k, n, ld["x"], ld["y"], env)
    if entry == "bwd":
        return P.plan_bwd(m, k, n, ld["x"], ld["y"], env, True, kw.pop("adds", False))
    return P.plan_bwd_bn(m, k, n, ld["x"], ld["y"], env, True, **kw)


def symbols(name, setting, entry, **kw):
    return set(geom(name, setting, entry, **kw)[0])


# -------------------------------------------------------------------------------------------------------------- the mirror
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ssdseglib import _hip
    if not os.path.exists(_hip.library_path()):
        g.build()
    return _hip.load_library()


def test_once_per_process_switch_is_unset():
    assert not [v for v in P.ONCE_ENV if v in os.environ]


SWEEP_M = (1, 127, 128, 129, 640, 16383, 16384, 16385, 65535, 65536, 65537, 65665, 131072, 149999, 150000, 499999, 500000, 2457600)
SWEEP_KN = ((16, 96), (64, 64), (96, 24), (24, 144), (160, 960), (256, 256), (576, 96), (56, 64), (60, 64), (1280, 256), (32, 32), (64, 36),
            (256, 36), (320, 32), (72, 512), (8, 64), (100, 164))
SWEEP_ENVS = ("default", "rowA", "resident", "tile", "tile-32", "tile-big", "scalar", "parts64")


def test_mirror_gives_the_librarys_table_rows_and_weight_copies(lib, monkeypatch):
    """ssdseg_pwconv_parts == rowA_grid_y and ssdseg_pwconv_wt_floats == pw_tile_wanted ? k n : 0 on both sides of every threshold
    (16,384, 65,536, 150,000 and 500,000 rows; 64 reduction channels and multiples of 8; 256 output channels), under every setting"""
    v = C.c_int()
    for setting in SWEEP_ENVS:
        env = P.SETTINGS[setting]
        for var in P.PW_VARS:
            monkeypatch.delenv(var, raising=False)
        for var, value in env.items():
            monkeypatch.setenv(var, value)
        for m in SWEEP_M:
            for k, n in SWEEP_KN:
                assert lib.ssdseg_pwconv_parts(m, n, C.byref(v)) == 0
                assert v.value == P.rowA_grid_y(m, n, env), (setting, m, n)
                for ldx in (k, k + 8):
                    assert lib.ssdseg_pwconv_wt_floats(m, ldx, k, n, C.byref(v)) == 0
                    assert v.value == (k * n if P.pw_tile_wanted(0, m, ldx, k, n, False, False, env) else 0), (setting, m, ldx, k, n)
    for name in P.CASES:
        m, k, n = P.shape_of(name)
        for var in P.PW_VARS:
            monkeypatch.delenv(var, raising=False)
        assert lib.ssdseg_pwconv_parts(m, n, C.byref(v)) == 0 and v.value == P.rowA_grid_y(m, n, {}), name


def _mirror_of_pinned_form(form, m, k, n, env):
    entry, _, what = form.partition(":")
    flags = what.split("+")
    if entry == "fwd_wt":
        return P.plan_fwd(m, k, n, k, env, wt_copy="copy" in flags)[0]
    if entry == "bwd_data":
        return P.plan_bwd_data(m, k, n, n, env, "bn" in flags, "adds" in flags)[0]
    if entry == "bwd":
        return P.plan_bwd(m, k, n, k, n, env, "bn" in flags, "adds" in flags)[0]
    if entry == "bwd_bn":
        return P.plan_bwd_bn(m, k, n, k, n, env, "bn" in flags)[0]
    return P.wgrad_plan(m, k, n, k, n, env)[0]


def test_mirror_names_the_pinned_instantiations():
    """the kernel symbols and launch counts the mirror expects against the table recorded in tests/test_gpu_pointwise_dispatch.py:
    every shape, operand form and kernel family of it"""
    import conftest
    import test_gpu_pointwise_dispatch as T
    envs = {f: {v: value for v, value in conftest.KERNEL_FAMILIES[f].items() if v in P.PW_VARS} for f in T.FAMILIES}
    checked = 0
    for (form, m, k, n), per_family in T.EXPECTED.items():
        for families, want in per_family.items():
            for family in families.split():
                assert _mirror_of_pinned_form(form, m, k, n, envs[family]) == want, (form, m, k, n, family)
                checked += 1
    assert checked == len(T.FORMS) * len(T.ROWS) * len(T.FAMILIES)


# ------------------------------------------------------------------------------------------------ the geometry of the cases
def test_every_case_reaches_the_kernel_it_is_there_for():
    for name, case in P.CASES.items():
        seen = set()
        for setting in case["settings"]:
            for entry in case["entries"]:
                seen |= symbols(name, setting, entry)
                if entry == "bwd_data":
                    seen |= symbols(name, setting, entry, adds=True)
        assert any(s.startswith(case["kernel"]) for s in seen), (name, case["kernel"], sorted(seen))


def test_row_cases_have_the_tiles_they_are_named_for():
    for m in (1, 31, 32, 33, 127, 128, 129, 255, 256, 257):
        g = geom(f"rows{m}-16x96", "rowA", "fwd")[1]
        assert g["row_tiles"] == P.cdiv(m, 128) and g["last_rows"] == (m - 1) % 128 + 1 and g["gy"] == g["row_tiles"]
        assert P.cdiv(m, 32) == {1: 1, 31: 1, 32: 1, 33: 2}.get(m, P.cdiv(m, 32))          # wave tiles of the resident kernel
        launches, g = geom(f"rows{m}-64x64", "tile-big", "fwd")
        assert "pw_tile_kernel<8, 2, 0>" in launches and g["block_rows"] == 256 and g["row_tiles"] == P.cdiv(m, 256), (m, launches)
        assert g["last_rows"] == (m - 1) % 256 + 1
        assert "pw_tile_kernel<4, 1, 0>" in geom(f"rows{m}-64x64", "tile", "fwd")[0]
        assert "pw_tile_kernel<8, 2, 1>" in geom(f"rows{m}-64x64", "tile-big", "bwd_data")[0]
        assert "gemm_wres_kernel<1, 0, 0>" in geom(f"rows{m}-64x64", "resident", "fwd")[0]
    assert geom("rows257-64x64", "tile-big", "fwd")[1]["last_rows"] == 1 and geom("rows129-16x96", "rowA", "fwd")[1]["last_rows"] == 1


def test_reduction_cases_sit_around_the_step_lengths():
    for r in (4, 28, 32, 36, 60, 64, 68):
        assert symbols(f"red-k{r}", "rowA", "fwd") == {"gemm_rowA_kernel<1, 0, 0, 0, 0, 0>"}
        assert symbols(f"red-k{r}", "resident", "fwd") == {"gemm_wres_kernel<1, 0, 0>"}
        assert symbols(f"red-n{r}", "rowA", "bwd_data") == {"gemm_rowA_kernel<1, 1, 0, 0, 0, 0>"}
        assert symbols(f"red-n{r}", "resident", "bwd_data") == {"gemm_wres_kernel<1, 1, 0>"}
    assert sorted({P.cdiv(r, 32) for r in (4, 28, 32, 36, 60, 64, 68)}) == [1, 2, 3]
    for r in (56, 60):
        assert symbols(f"tile-k{r}", "tile", "fwd") == {"gemm_rowA_kernel<1, 0, 0, 0, 0, 0>"}
        assert "gemm_rowA_kernel<1, 1, 0, 0, 0, 0>" in symbols(f"tile-n{r}", "tile", "bwd_data")
    for r in (64, 72, 96, 104):
        assert symbols(f"tile-k{r}", "tile", "fwd") == {"pw_tile_kernel<4, 1, 0>", "conv3_transpose_w_kernel"}
        assert symbols(f"tile-n{r}", "tile", "bwd_data") == {"pw_tile_kernel<4, 1, 1>"}
        assert "pw_tile_kernel<4, 1, 1>" in symbols(f"tile-n{r}", "tile", "bwd_bn")
    assert [(r // 32, r % 32) for r in (64, 72, 96, 104)] == [(2, 0), (2, 8), (3, 0), (3, 8)]
    assert P.wres_lds_bytes(288, 1) > 0 and P.wres_lds_bytes(320, 1) == 0 and P.wres_lds_bytes(289, 1) == 0
    assert symbols("fit-288", "resident", "fwd") == {"gemm_wres_kernel<1, 0, 0>"}
    assert symbols("fit-320", "resident", "fwd") == {"gemm_rowA_kernel<1, 0, 0, 0, 0, 0>"}


def test_column_cases_have_the_ragged_tiles_they_are_named_for():
    for n in (4, 28, 32, 36, 100, 160, 164):
        g = geom(f"cols{n}", "rowA", "fwd")[1]
        assert g["wn"] == 1 and g["gx"] == P.cdiv(n, 32) and g["last_cols"] == (n - 1) % 32 + 1       # two row tiles: the narrowest tile
    want = {   # n: tile (ncols, column tiles), tile-32, tile-big (symbol, ncols, tiles)
        64: ((32, 2), (32, 2), ("pw_tile_kernel<8, 2, 0>", 64, 1)), 128: ((32, 4), (32, 4), ("pw_tile_kernel<8, 4, 0>", 128, 1)),
        160: ((32, 5), (32, 5), ("pw_tile_kernel<8, 5, 0>", 160, 1)), 192: ((32, 6), (32, 6), ("pw_tile_kernel<8, 6, 0>", 192, 1)),
        256: ((32, 8), (32, 8), ("pw_tile_kernel<8, 8, 0>", 256, 1)), 260: ((32, 9), (32, 9), ("pw_tile_kernel<8, 5, 0>", 132, 2))}
    for n, (tile, tile32, big) in want.items():
        for setting, (ncols, tiles) in (("tile", tile), ("tile-32", tile32)):
            launches, g = geom(f"tcols{n}", setting, "fwd")
            assert "pw_tile_kernel<4, 1, 0>" in launches and (g["ncols"], g["gx"]) == (ncols, tiles), (n, setting, g)
        launches, g = geom(f"tcols{n}", "tile-big", "fwd")
        assert big[0] in launches and (g["ncols"], g["gx"]) == big[1:], (n, launches, g)
    assert geom("tcols260", "tile-32", "fwd")[1]["last_cols"] == 4 and geom("tcols260", "tile-big", "fwd")[1]["last_cols"] == 128


def test_grid_cases_take_the_4x2_wave_grid():
    want = {164: "pw_tile_kernel<8, 3, 1, 2>", 200: "pw_tile_kernel<8, 4, 1, 2>", 256: "pw_tile_kernel<8, 4, 1, 2>"}
    for m in (129, 257):
        for k, symbol in want.items():
            launches, g = geom(f"grid42-{m}x{k}", "tile-big", "bwd_data")
            assert launches == {symbol: 1} and g["grid42"] and g["block_rows"] == 128 and g["gx"] == 1 and g["last_rows"] == 1
            assert symbol in symbols(f"grid42-{m}x{k}", "tile-big", "bwd_bn")
            launches, g = geom(f"grid42-{m}x{k}", "tile-big-nogrid", "bwd_data")
            assert not g["grid42"] and g["gx"] == 2 and g["block_rows"] == 256, (m, k, launches)
    # the second wave group of the grid holds the columns from 32 * WN on: 164 - 96 = 68 = 2 tiles + 4 ... the ragged remainders
    assert (164 - 96) % 32 == 4 and (200 - 128) % 32 == 8 and (256 - 128) % 32 == 0


def test_wide_cases_reach_every_width_epilogue_and_occupancy_form():
    seen = set()
    for n, wn in ((60, 2), (64, 2), (92, 3), (96, 3), (100, 4), (128, 4), (160, 5)):
        g = geom(f"wide-n{n}", "rowA", "fwd")[1]
        assert g["wn"] == wn and g["row_tiles"] == 514 and g["last_rows"] == 1 and g["gy"] == 514, (n, g)
        for setting in P.settings_of(f"wide-n{n}"):
            seen |= symbols(f"wide-n{n}", setting, "fwd") | symbols(f"wide-k{n}", setting, "bwd_data") | symbols(f"wide-k{n}", setting, "bwd_bn")
            seen |= symbols(f"wide-k{n}", setting, "bwd_data", adds=True)
        assert geom(f"wide-k{n}", "rowA", "bwd_data")[1]["wn"] == wn
        assert geom(f"wide-k{n}", "rowA-occ", "bwd_data")[1]["wn"] == min(wn, 3)        # the SSDSEG_ROWA_BWD_WN cap: reduction 16 <= 48
        assert geom(f"wide-k{n}", "rowA-occ", "bwd_bn")[1]["wn"] == min(wn, 3)
        assert symbols(f"wide-n{n}", "resident", "fwd") == {f"gemm_wres_kernel<{wn}, 0, 0>"}
    for occ in (0, 1):
        for wn in (2, 3, 4, 5):
            assert f"gemm_rowA_kernel<{wn}, 0, 0, 0, 1, {occ}>" in seen
        for wn in (2, 3) + ((4, 5) if occ == 0 else ()):
            assert f"gemm_rowA_kernel<{wn}, 1, 0, 0, 1, {occ}>" in seen and f"gemm_rowA_kernel<{wn}, 1, 0, 0, 2, {occ}>" in seen
    for wn in (2, 3, 4, 5):
        assert f"gemm_rowA_kernel<{wn}, 0, 0, 0, 0, 0>" in seen and f"gemm_rowA_kernel<{wn}, 1, 0, 0, 0, 0>" in seen      # `scalar`


def test_grid_stride_cases_walk_three_trips():
    launches, g = geom("stride-16x32", "parts64", "fwd")
    assert launches == {"gemm_rowA_kernel<1, 0, 0, 0, 0, 0>": 1} and g["row_tiles"] == 130 and g["last_rows"] == 1
    assert g["gy"] == g["nparts"] == 44 and P.cdiv(130, 44) == 3                    # 130 row tiles dealt three to a block
    launches, g = geom("stride-64x64", "parts64", "fwd", stats=True)
    assert "pw_tile_kernel<4, 2, 0>" in launches and g["gx"] == 1 and g["row_tiles"] == 130 and g["last_rows"] == 1
    assert g["gy"] == P.rowA_grid_y(16513, 64, P.SETTINGS["parts64"]) == 26           # one block per row of the statistics table:
    assert P.cdiv(130, 26) == 5                                                       # five trips, the last on the one-row tile
    launches, g = geom("stride-64x64", "parts64", "bwd_data", coef=True)
    assert launches == {"gemm_rowA_kernel<1, 1, 0, 0, 0, 0>": 1} and g["gy"] == 26 and g["gx"] == 2 and g["last_rows"] == 1


def test_fused_cases_have_the_chunk_counts_and_walks_they_are_named_for():
    for m in (1, 33, 129, 640):
        for (k, n), nt in zip(P.FUSED_KN, (1, 2, 2, 3, 4, 4, 5, 6)):
            name = f"fused-{m}x{k}x{n}"
            launches, g = geom(name, "resident", "bwd")
            assert g["symbol"] == f"gemm_wres_kernel<1, 1, {nt}>" and ("colsum_kernel" in launches) == (m > 128), (name, launches)
            assert geom(name, "rowA-fused", "bwd")[1]["symbol"] == f"gemm_rowA_kernel<1, 1, 0, {nt}, 0, 0>"
            assert geom(name, "rowA-fused-occ", "bwd")[1]["symbol"] == f"gemm_rowA_kernel<1, 1, 0, {nt}, 0, 1>"
        for k, n in ((36, 96), (16, 196)):
            for setting in ("resident", "rowA-fused"):
                launches, g = geom(f"unfused-{m}x{k}x{n}", setting, "bwd")
                assert g is None and not any(", 1, 0, 1," in s or s.startswith("gemm_wres_kernel<1, 1, ") and not s.endswith(", 0>") for s in launches)
    for (k, n), nt in (((8, 64), 2), ((16, 96), 3), ((32, 128), 4)):
        g = geom(f"fused-walk-{k}x{n}", "resident", "bwd")[1]
        assert g["symbol"] == f"gemm_wres_kernel<1, 1, {nt}>" and (g["tiles"], g["walkers"], g["second_trip"], g["trips"]) == (2053, 2048, 5, 2)
        assert 65669 - 2052 * 32 == 5                                                # the last wave tile is ragged
    for (k, n), nt in (((16, 96), 3), ((24, 160), 5)):
        g = geom(f"fused-walk-occ-{k}x{n}", "rowA-fused-occ", "bwd")[1]
        assert g["symbol"] == f"gemm_rowA_kernel<1, 1, 0, {nt}, 0, 1>" and (g["tiles"], g["walkers"], g["second_trip"]) == (514, 512, 2)


def test_weight_gradient_cases_reach_every_tile_shape_and_split_edge():
    reached = set()
    for name, case in P.CASES.items():
        if not name.startswith("wgrad-") or name.startswith("wgrad-general"):
            continue
        m, k, n = case["shape"]
        launches, g = geom(name, "default", "bwd_weight")
        assert g["row_naming"] and g["symbol"].startswith(case["kernel"]), (name, g)
        reached.add(g["symbol"])
        assert ("colsum_kernel" in launches) == (g["splits"] > 1)
        tag = name.split("-")[-1]
        if "-edge-" in name:
            assert k % g["kt"] == 4 or g["kt"] > k, (name, g)
            assert g["ktiles"] * g["kt"] - k > 0 and g["ntiles"] * g["nt"] - n > 0
        elif tag == "m1":
            assert g["steps"] == 1 and g["splits"] == 1 and g["last_split_rows"] == 1
        elif m == g["ms"] - 1 or m == g["ms"] + 1:
            assert g["steps"] == (1 if m < g["ms"] else 2) and g["splits"] == 1
        elif g["last_split_rows"] == g["rows_per_split"]:
            assert g["splits"] >= 2 and m % g["ms"] == 0                              # the step prefetched past the split is another split's
        else:
            assert g["splits"] >= 2 and (m - 1) % g["ms"] == 0                        # one row beyond a whole number of steps
    assert reached == {"pw_wgrad_kernel<%d, %d, %d, %d>" % inst for _, _, inst in P.PWW_SHAPES}
    whole = [n for n in P.CASES if n.startswith("wgrad-") and "-edge-" not in n and not n.startswith("wgrad-general")]
    for inst in {n.split("-")[1] for n in whole}:
        ms_cases = sorted((P.shape_of(n)[0] for n in whole if n.split("-")[1] == inst))
        g0 = geom(f"wgrad-{inst}-m{ms_cases[3]}", "default", "bwd_weight")[1]
        g1 = geom(f"wgrad-{inst}-m{ms_cases[4]}", "default", "bwd_weight")[1]
        assert g0["splits"] >= 2 and g0["last_split_rows"] == g0["rows_per_split"]
        assert ms_cases[4] == ms_cases[3] + 1 and g1["splits"] >= 2 and (g1["last_split_rows"] - 1) % g1["ms"] == 0    # a split (or step) of one row
    for (k, n), symbol in (((16, 36), "gemm_wgrad_kernel<1, 4, "), ((48, 100), "gemm_wgrad_kernel<2, 2, "), ((100, 164), "gemm_wgrad_kernel<4, 1, ")):
        launches, g = geom(f"wgrad-general-{k}x{n}", "rowA", "bwd_weight")
        assert g["symbol"].startswith(symbol) and g["splits"] in (3, 4) and launches.get("colsum_kernel") == 1, (k, n, g)
        assert 0 < g["last_split_rows"] < g["rows_per_split"] and g["last_split_rows"] % g["ms"] != 0          # a ragged last split and step
        assert k % g["kt"] != 0 and n % g["nt"] != 0


def test_pitch_and_unaligned_cases():
    for name in P.CASES:
        ld = P.CASES[name]["ld"]
        if ld:
            m, k, n = P.shape_of(name)
            assert ld["x"] > k and ld["y"] > n and ld["dx"] > k and ld["r"] > k and all(v % 4 == 0 for v in ld.values())
    assert "pw_tile_kernel<4, 1, 0>" in symbols("pitch-130x64x64", "tile", "fwd") and symbols("pitch-130x48x64", "tile", "fwd") == {"gemm_rowA_kernel<1, 0, 0, 0, 0, 0>"}
    env = P.SETTINGS["rowA"]
    # the aligned call of the 514-tile shapes leaves through the float4 / BatchNorm epilogue, the unaligned one through the scalar one
    assert P.plan_fwd(65665, 16, 96, 16, env)[0] == {"gemm_rowA_kernel<3, 0, 0, 0, 1, 0>": 1}
    assert P.plan_fwd(65665, 16, 96, 16, env, aligned=False)[0] == {"gemm_rowA_kernel<3, 0, 0, 0, 0, 0>": 1}
    assert P.plan_bwd_data(65665, 96, 16, 16, env, True, True)[0] == {"gemm_rowA_kernel<3, 1, 0, 0, 1, 0>": 1}
    assert P.plan_bwd_data(65665, 96, 16, 16, env, True, True, aligned=False)[0] == {"gemm_rowA_kernel<3, 1, 0, 0, 0, 0>": 1}
    for m, k, n, wn in ((65665, 96, 16, 3), (130, 96, 24, 1)):
        fused, plain = P.plan_bwd_bn(m, k, n, k, n, env, True)[0], P.plan_bwd_bn(m, k, n, k, n, env, True, aligned=False)[0]
        assert fused[f"gemm_rowA_kernel<{wn}, 1, 0, 0, 2, 0>"] == 1 and "bn_bwd_partial_kernel" not in fused
        assert plain[f"gemm_rowA_kernel<{wn}, 1, 0, 0, 0, 0>"] == 1 and plain["bn_bwd_partial_kernel"] == 1 and plain["bn_bwd_finalize_kernel"] == 1
    # (two row tiles never reach a column tile of two: the small shapes take the scalar epilogue either way, and must give the same values)
    assert P.plan_fwd(130, 16, 96, 16, env)[0] == P.plan_fwd(130, 16, 96, 16, env, aligned=False)[0] == {"gemm_rowA_kernel<1, 0, 0, 0, 0, 0>": 1}
    for name, setting in P.TRANSPOSED:
        tile = any(s.startswith("pw_tile_kernel") for s in symbols(name, setting, "fwd"))
        assert tile == (name != "tile-k60")


# ----------------------------------------------------------------------------------------------------------- exactness
def _f32(a):
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


@pytest.mark.parametrize("name", list(P.CASES))
def test_lattice_case_is_exact_and_not_degenerate(name):
    k = P.lattice_case(name)
    m, kk, n = k.shape
    b = P.budget(k)
    assert max(b.values()) < P.EXACT, (name, k.mode, b)
    rng = P.seeded(5, m, kk, n)
    pk, pn, pm = rng.permutation(kk), rng.permutation(n), rng.permutation(m)
    large = P.CASES[name]["forms"] == "large"
    views = (O.ACT_RELU6,) if large else ("plain", O.ACT_RELU6, O.ACT_NONE)
    w32 = k.w
    for view in views:
        y, s, q = P.ref_fwd(k, view)
        assert np.array_equal(_f32(y), y) and np.array_equal(_f32(s), s) and np.array_equal(_f32(q), q)
        a32 = P.in_view(k, view, F32)[0]
        y32 = a32[:, pk] @ w32[pk]
        assert y32.dtype == F32 and np.array_equal(y32.astype(np.float64), y)
        assert np.array_equal(y32[pm].sum(axis=0, dtype=F32).astype(np.float64), s)
        assert np.array_equal((y32 * y32)[pm].sum(axis=0, dtype=F32).astype(np.float64), q)
        # (65,000 rows and more: the one form the case runs -- the conv's own output in the gradient view where it runs ssdseg_pwconv_bwd)
        for gview, own in ((O.ACT_RELU6, "bwd" in P.CASES[name]["entries"]),) if large else ((O.ACT_RELU6, False), (O.ACT_NONE, True), ("identity", False)):
            yv = P.own_y(k, view) if own else None
            dx = P.ref_dx(k, gview, 1, 1, y=yv)
            dw = P.ref_dw(k, view, gview, y=yv)
            assert np.array_equal(_f32(dx), dx) and np.array_equal(_f32(dw), dw)
            dy32 = P.g_view(k, gview, F32, y=yv)
            assert dy32.dtype == F32 and np.array_equal(dy32.astype(np.float64), P.g_view(k, gview, y=yv))
            dx32 = dy32[:, pn] @ w32.T[pn] + k.res + k.base
            assert np.array_equal(dx32.astype(np.float64), dx)
            assert np.array_equal((a32[pm].T @ dy32[pm]).astype(np.float64), dw)
        if view != "plain" and not (large and "bwd_bn" not in P.CASES[name]["entries"]):
            r = P.ref_bn(k, view, O.ACT_RELU6)
            for v in r[:4]:
                assert np.array_equal(_f32(v), v)
            _, mask = P.in_view(k, view, F32)
            dx32 = (P.g_view(k, O.ACT_RELU6, F32) @ w32.T) * mask
            xhat32 = (k.x - k.mean) * k.invstd
            assert np.array_equal(dx32[pm].sum(axis=0, dtype=F32).astype(np.float64), r[3])
            assert np.array_equal((dx32 * xhat32)[pm].sum(axis=0, dtype=F32).astype(np.float64), r[2])
    # the last row, the last float4 of the reduction and the last column each carry a non-zero term of y, dx and dW
    x, w, g = (v.astype(np.float64) for v in (k.x, k.w, k.g))
    assert x[-1, -1] * w[-1, -1] != 0 and (x[-1, kk - 4:] * w[kk - 4:, -1]).any()          # y[-1, -1]: last row, last vector, last column
    assert g[-1, -1] * w[-1, -1] != 0 and (g[-1, n - 4:] * w[-1, n - 4:]).any()            # dx[-1, -1]
    assert x[-1, -1] * g[-1, -1] != 0                                                      # dW[-1, -1]: the last row's term
    assert k.res.any() and k.base.any()


@pytest.mark.parametrize("name", [n for n in SMALL if P.shape_of(n)[0] >= 100])
def test_both_thresholds_are_hit_in_both_views(name):
    k = P.lattice_case(name)
    if k.mode == "sparse":
        return              # no shifts on the sparse lattice: named in the module docstring
    m, kk, n = k.shape
    zi = k.x.astype(np.float64) * k.scale + k.shift
    zg = k.yraw.astype(np.float64) * k.gscale + k.gshift
    for z in (zi, zg):
        if z.size >= 400:
            assert (z == 0).mean() >= 0.01 and (z == 6).mean() >= 0.01, (name, (z == 0).mean(), (z == 6).mean())
    for z in (zi, zg):
        mask = O.act_mask(z, O.ACT_RELU6)
        for ch in range(z.shape[1]):
            assert 0 < mask[:, ch].sum() < m, (name, ch)


# ------------------------------------------------------------------------------------- structural errors move the reference
def units(k):
    """lattice units of (y, dx, dW)"""
    xd, wd = float(k.xd), float(k.wd)
    return 1 / (xd * wd), 1 / (xd * xd * wd), 1 / xd ** 3


def moved(a, b, unit):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) >= unit


STRUCT = ["rows129-16x96", "rows257-64x64", "red-k36", "red-n68", "tile-k72", "tile-n104", "cols164", "cols-k100", "tcols260", "grid42-257x164",
          "fused-129x28x100", "fused-640x32x192", "wgrad-general-48x100", "pitch-130x48x64", "stride-16x32"]


@pytest.mark.parametrize("name", STRUCT)
def test_structural_errors_move_the_reference(name):
    k = P.lattice_case(name)
    m, kk, n = k.shape
    uy, udx, udw = units(k)
    w = k.w.astype(np.float64)
    for view, gview in (("plain", "identity"), (O.ACT_RELU6, O.ACT_RELU6)):
        a, _ = P.in_view(k, view)
        dy = P.g_view(k, gview)
        y, s, q = P.ref_fwd(k, view)
        dx, dw = P.ref_dx(k, gview, 1, 1), P.ref_dw(k, view, gview)
        # the last row dropped: its statistics terms and its dW term
        if view == "plain":
            assert moved(y[:-1].sum(axis=0), s, uy) and moved(a[:-1].T @ dy[:-1], dw, udw)
            # the last reduction vector dropped
            assert moved(a[:, :kk - 4] @ w[:kk - 4], y, uy) and moved(dy[:, :n - 4] @ w[:, :n - 4].T, P.ref_dx(k, gview), udx)
        # the last column tile dropped (left unwritten, or taken as zero)
        assert np.abs(y[:, -1]).max() >= uy or view != "plain"
        assert np.abs(dw[:, -1]).max() >= udw or view != "plain"
        # the residual or the accumulation base skipped
        assert moved(P.ref_dx(k, gview, 0, 1), dx, udx) and moved(P.ref_dx(k, gview, 1, 0), dx, udx)
    # `>=` for `>` at a threshold: the gradient view's mask, and the producer's mask in the fused sums
    if k.mode != "sparse":
        assert moved(P.ref_dx(k, O.ACT_RELU6, gview_nonstrict=True), P.ref_dx(k, O.ACT_RELU6), udx)
        strict, loose = P.ref_bn(k, O.ACT_RELU6, "identity"), P.ref_bn(k, O.ACT_RELU6, "identity", view_nonstrict=True)
        assert moved(loose[3], strict[3], udx) or moved(loose[2], strict[2], udx / (2 * k.xd))
    # the row past a split counted: the general weight gradient's and the row-naming kernel's split edges
    rps = P.wgrad_plan(m, kk, n, kk, n, {})[1]["rows_per_split"]
    if rps < m:
        extra = np.outer(k.x[rps].astype(np.float64), k.g[rps].astype(np.float64))
        assert np.abs(extra).max() >= udw or not k.x[rps].any() or not k.g[rps].any()
    # a gap column read: the guarded inputs hold a NaN there, which no product hides
    assert np.isnan(np.float32(np.nan) * F32(0))


def test_split_edge_rows_are_not_empty():
    """counting the row past a split must move dW: in every whole-splits weight-gradient case the first row of the second split has
    a non-zero x and a non-zero g"""
    n_checked = 0
    for name in P.CASES:
        if not name.startswith("wgrad-") or P.shape_of(name)[0] < 100:
            continue
        m, kk, n = P.shape_of(name)
        g = P.wgrad_plan(m, kk, n, kk, n, P.SETTINGS[P.settings_of(name)[0]])[1]
        if g["splits"] < 2:
            continue
        k = P.lattice_case(name)
        row = g["rows_per_split"]
        assert np.abs(np.outer(k.x[row], k.g[row])).max() > 0, name
        n_checked += 1
    assert n_checked >= 26


def test_normal_bounds_are_positive_and_small():
    for name in P.NORMAL_CASES:
        k = P.normal_case(name)
        b = P.normal_bounds(k, O.ACT_RELU6, O.ACT_RELU6, 1, 1)
        y, _, _ = P.ref_fwd(k, O.ACT_RELU6)
        assert (b["y"] > 0).all() and b["y"].max() < 1e-3 * max(np.abs(y).max(), 1)
        z = np.concatenate([(k.x.astype(np.float64) * k.scale + k.shift).ravel(), (k.yraw.astype(np.float64) * k.gscale + k.gshift).ravel()])
        assert (np.abs(z) >= P.BAND * 0.99).all() and (np.abs(z - 6) >= P.BAND * 0.99).all()
