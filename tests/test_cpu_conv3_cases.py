"""The reference, the cases and the mirror of tests/_conv3_cases.py, vetted without a GPU: the float64 reference against torch's conv2d
with autograd in float64 (y, dx, dW under both views); every lattice case below 2^24 in every budgeted reduction, the transformed
domains of F(2x2, 3x3) and of the Winograd weight gradient included, and hitting both activation thresholds in both views; every
case with the geometric property it is named for, by the mirror; the mirror of ssdseg_conv3x3_parts and ssdseg_conv3x3_saved_floats
against the library's host functions (they run without a device); the even deal of the Winograd weight gradient and the split-K
arithmetic at three CU counts; the F(4x4, 3x3) bound against a float32 NumPy emulation of the three transforms -- inside the bound on
every F(4x4) case in both families, outside it once one tap weight of one channel is off by 2^-10 relative."""
import ctypes as C
import os

import numpy as np
import pytest

import _conv3_cases as P
from oracle import np_ops as O

F32 = np.float32
CU_COUNTS = (256, 304, 64)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ssdseglib import _hip
    if not os.path.exists(_hip.library_path()):
        g.build()
    return _hip.load_library()


def use(monkeypatch, env):
    for v in P.CONV3_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, value in env.items():
        monkeypatch.setenv(v, value)


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name,family", [("px-9x33", "lattice"), ("px-7x31", "normal"), ("gemm-straddle", "lattice"), ("narrow-16x4", "normal"),
                                         ("ww-tail-two", "lattice"), ("f4-plain", "normal")])
def test_reference_agrees_with_torch_autograd_in_float64(name, family):
    import torch
    import torch.nn.functional as TF
    k = P.lattice_case(name) if family == "lattice" else P.normal_case(name)
    for view, gview in (("plain", "identity"), (O.ACT_RELU6, O.ACT_RELU6), (O.ACT_RELU, "identity"), (O.ACT_NONE, O.ACT_RELU)):
        a = torch.tensor(P.in_view(k, view)[0].transpose(0, 3, 1, 2).copy(), dtype=torch.float64, requires_grad=True)
        wt = torch.tensor(k.w.astype(np.float64).transpose(3, 2, 0, 1).copy(), requires_grad=True)
        y = TF.conv2d(a, wt, padding=1)
        y.backward(torch.tensor(P.g_view(k, gview).transpose(0, 3, 1, 2).copy()))
        y_ref, s_ref, q_ref = P.ref_fwd(k, view)
        scale = max(np.abs(y_ref).max(), 1.0)
        assert np.abs(y.detach().numpy().transpose(0, 2, 3, 1) - y_ref).max() <= 1e-12 * scale
        assert np.allclose(s_ref, y_ref.sum(axis=(0, 1, 2))) and np.allclose(q_ref, (y_ref ** 2).sum(axis=(0, 1, 2)))
        dx_ref, dw_ref = P.ref_dx(k, gview), P.ref_dw(k, view, gview)
        assert np.abs(a.grad.numpy().transpose(0, 2, 3, 1) - dx_ref).max() <= 1e-12 * max(np.abs(dx_ref).max(), 1.0)
        assert np.abs(wt.grad.numpy().transpose(2, 3, 1, 0) - dw_ref).max() <= 1e-12 * max(np.abs(dw_ref).max(), 1.0)
        assert np.array_equal(P.ref_dx(k, gview, 1), dx_ref + k.base.astype(np.float64))
    # the fused BatchNorm sums, written out from their definitions
    dx, dgamma, dbeta, k1, k0, _ = P.ref_bn(k, O.ACT_RELU6, "identity")
    x = k.x.astype(np.float64)
    z = x * k.scale + k.shift
    inside = (z > 0) & (z < 6)
    m = x.shape[0] * x.shape[1] * x.shape[2]
    assert np.allclose(dbeta, np.where(inside, dx, 0).sum(axis=(0, 1, 2)))
    assert np.allclose(dgamma, np.where(inside, dx * (x - k.mean) * k.invstd, 0).sum(axis=(0, 1, 2)))
    assert np.allclose(k1, -k.scale * dgamma * k.invstd / m) and np.allclose(k0, k.scale * (dgamma * k.invstd * k.mean - dbeta) / m)


def test_winograd_in_float64_is_the_convolution():
    """the NumPy F(2x2) and F(4x4) forms (the emulation, the budgets and the bound are built on them) equal the direct sum, both roles"""
    k = P.normal_case("f4-plain")
    y = P.ref_fwd(k, O.ACT_RELU6)[0]
    a = P.in_view(k, O.ACT_RELU6)[0]
    for mats in (P.F2, P.F4):
        assert np.abs(P.winograd(a, k.w, mats) - y).max() <= 1e-11 * np.abs(y).max()
        dx = P.winograd(k.g.astype(np.float64), P.flipped(k.w.astype(np.float64)), mats)
        assert np.abs(dx - P.ref_dx(k, "identity")).max() <= 1e-11 * np.abs(dx).max()


# ------------------------------------------------------------------------------------------------------- lattice: budgets
@pytest.mark.parametrize("name", list(P.CASES))
def test_lattice_case_is_exact_and_not_degenerate(name):
    k = P.lattice_case(name)
    n, h, w, cin, cout = k.shape
    b = P.budget(k)
    assert set(P.MUST_HOLD) < set(b) and P.holds(b), {q: v for q, v in b.items() if v >= P.EXACT}
    # on the lattice: x, g, yraw, shifts, k1, k0, mean multiples of 1 / xd, weights of 1 / wd, scales and invstd signed powers of two
    for a, den in ((k.x, k.xd), (k.g, k.xd), (k.yraw, k.xd), (k.base, k.xd), (k.shift, k.xd), (k.gshift, k.xd), (k.k1, k.xd), (k.k0, k.xd),
                   (k.mean, k.xd), (k.w, k.wd)):
        assert np.array_equal(a * den, np.round(a * den))
    for s in (k.scale, k.gscale, k.invstd):
        assert np.array_equal(np.abs(s), 2.0 ** np.round(np.log2(np.abs(s))))
    # the float64 reference is a float32 number everywhere: the bound is 0
    for view, gview in ((O.ACT_RELU6, O.ACT_RELU6), ("plain", "identity")):
        for ref in (P.ref_fwd(k, view)[0], P.ref_dx(k, gview, 1), P.ref_dw(k, view, gview)):
            assert np.array_equal(ref.astype(F32).astype(np.float64), ref)
    # every tap and both ends of the channel range matter: dropping any of them moves the reference
    y = P.ref_fwd(k, "plain")[0]
    live = np.outer([h > 1, True, h > 1], [w > 1, True, w > 1])          # (a one-row image never meets the taps above and below)
    assert y.any() and np.array_equal(P.ref_dw(k, "plain", "identity").any(axis=(2, 3)), live)
    for c in (0, cin - 1):
        assert k.x[..., c].any() and k.w[:, :, c, :].any(axis=2).all()
    assert k.w[:, :, :, cout - 1].any(axis=2).all() and k.g[..., cout - 1].any()


@pytest.mark.parametrize("name", list(P.CASES))
def test_both_thresholds_are_hit_in_both_views(name):
    k = P.lattice_case(name)
    n, h, w, cin, cout = k.shape
    z = k.x.astype(np.float64) * k.scale + k.shift
    zg = k.yraw.astype(np.float64) * k.gscale + k.gshift
    count = n * h * w * min(cin, cout)
    need = 0 if count < 64 else (1 if count < 512 else 2)        # (a one-pixel case has too few values to promise a hit)
    for pre in (z, zg):
        assert (pre == 0).sum() >= need and (pre == 6).sum() >= need, (name, int((pre == 0).sum()), int((pre == 6).sum()))
    if need:
        # a threshold counted as inside would move the reference
        loose = ((z >= 0) & (z <= 6)).astype(np.float64)
        assert not np.array_equal(loose, O.act_mask(z, O.ACT_RELU6))
        dx = P.ref_dx(k, "identity")
        if "bwd_data_bn" in P.CASES[name]["entries"] and (dx * (loose - O.act_mask(z, O.ACT_RELU6))).any():
            assert not np.array_equal((dx * loose).sum(axis=(0, 1, 2)), P.ref_bn(k, O.ACT_RELU6, "identity")[2])


def test_at_least_one_exact_sum_of_squares_per_forward_family():
    """where the sum of y^2 over all pixels stays below 2^24 units of the squared lattice, every statistics row is exact and the GPU
    file demands the fold bit for bit; elsewhere it bounds it"""
    exact = {}
    for name, case in P.CASES.items():
        if "fwd" not in case["entries"] and name not in P.SAVED:
            continue
        if P.budget(P.lattice_case(name))["sumsq"] < P.EXACT:
            for setting in case["settings"]:
                exact.setdefault(P.fwd_plan(P.SETTINGS[setting], *case["shape"][:3], P.ldx_of(name), *case["shape"][3:])["family"], name)
    assert set(exact) >= {"tile", "wino", "wino4", "gemm", "narrow"}, exact


# ---------------------------------------------------------------------------------------------- the mirror and the library
def test_mirror_gives_the_librarys_table_rows_and_saved_sizes(lib, monkeypatch):
    shapes = [c["shape"] for c in P.CASES.values()] + [(2, 9, 11, 16, 32), (1, 12, 16, 304, 256), (256, 8, 32, 16, 64), (1024, 4, 4, 64, 64),
                                                       (32, 120, 160, 304, 256), (32, 60, 80, 304, 256), (3, 14, 40, 72, 96), (2, 13, 18, 48, 80)]
    v, f = C.c_int(), C.c_longlong()
    for setting, env in P.SETTINGS.items():
        use(monkeypatch, env)
        for s in shapes:
            assert lib.ssdseg_conv3x3_parts(*s, C.byref(v)) == 0 and v.value == P.fwd_table_rows(*s), (setting, s)
            assert lib.ssdseg_conv3x3_saved_floats(*s, C.byref(f)) == 0 and f.value == P.saved_floats(env, *s), (setting, s)
            # the table holds the rows of whichever forward kernel the switches pick
            assert P.fwd_plan(env, *s[:3], s[3], *s[3:])["rows"] <= v.value
    for bad, arg in (((0, 4, 4, 8, 8), 1), ((1, 4, 4, 6, 8), 4), ((1, 4, 4, 8, 0), 5)):
        assert lib.ssdseg_conv3x3_parts(*bad, C.byref(v)) == -1000 - arg and lib.ssdseg_conv3x3_saved_floats(*bad, C.byref(f)) == -1000 - arg
    assert lib.ssdseg_conv3x3_parts(1, 4, 4, 8, 8, None) == -1006 and lib.ssdseg_conv3x3_saved_floats(1, 4, 4, 8, 8, None) == -1006


def test_every_case_reaches_the_kernel_it_is_there_for():
    seen = set()
    for name, case in P.CASES.items():
        for setting in case["settings"]:
            for entry in case["entries"]:
                for form in P.forms_of(name, entry):
                    seen.add(P.expected_kernel(name, setting, entry, form))
    # (expected_kernel gives patterns: the symbols they stand for)
    symbols = [f"conv3_tile_kernel<{wn}> [{r}]" for wn in range(1, 6) for r in ("fwd", "bwd_data")] + \
        [f"{kn}<{v}> [{r}]" for kn in ("conv3_wino_kernel", "conv3_wino4_kernel") for v, r in (("true", "fwd"), ("false", "fwd"), ("false", "bwd_data"))] + \
        ["conv3_wino_wgrad_kernel", "conv3_wgrad_tile_kernel", "conv3_wgrad12_kernel", "(conv3_wgrad9_kernel<1>)", "(conv3_wgrad9_kernel<4>)", "conv3n_tapsum_kernel",
         "conv3n_shift_kernel", "conv3n_bwd_bn_direct_kernel", "gemm_rowA_kernel<1, 0, 1, 0, 0, 0>", "gemm_rowA_kernel<1, 1, 1, 0, 0, 0>",
         "gemm_wgrad_kernel<1, 4, 1> [conv3x3 tap]"]
    for s in symbols:
        assert any(P.reaches([s], pattern) for pattern in seen), s


def test_pixel_tile_cases():
    g = lambda name: P.conv3t_geometry(*P.shape_of(name)[:3], P.shape_of(name)[4])      # noqa: E731
    assert P.shape_of("px-1x1") == (1, 1, 1, 8, 8) and g("px-1x1")["mtiles"] == 1
    assert g("px-8x32")["mtiles"] == 1 and P.shape_of("px-8x32")[1:3] == (P.C3T_ROWS, P.C3T_COLS)
    n, h, w = P.shape_of("px-9x33")[:3]
    assert n == 2 and (g("px-9x33")["tiles_h"], g("px-9x33")["tiles_w"]) == (2, 2) and h % P.C3T_ROWS == 1 and w % P.C3T_COLS == 1
    n, h, w = P.shape_of("px-7x31")[:3]
    assert n == 2 and g("px-7x31")["mtiles"] == 2 and h == P.C3T_ROWS - 1 and w == P.C3T_COLS - 1 and h % 2 == 1 and w % 2 == 1
    for name in ("px-1x1", "px-8x32", "px-9x33", "px-7x31"):
        for entry, form in (("fwd", ("plain", True)), ("bwd_data", ("identity", 0, False)), ("bwd_weight", ("plain", "identity"))):
            assert P.plan_of(name, "default", entry, form)["family"] == "tile"
            assert P.plan_of(name, "wino", entry, form)["family"] == ("wino" if entry != "bwd_weight" or (P.shape_of(name)[1] % 2 == 0 and P.shape_of(name)[2] % 2 == 0) else "tile")
        # a halo row of one image is a row of the next in memory: only a mask keeps it out
        assert P.plan_of(name, "default", "bwd_data", (O.ACT_RELU6, 0, False))["family"] == "gemm"


def test_column_tile_cases():
    for nout, wn in P.COL_NOUT.items():
        for name, entry, form in ((f"col-fwd-{nout}", "fwd", ("plain", True)), (f"col-bwd-{nout}", "bwd_data", ("identity", 0, False))):
            p = P.plan_of(name, "default", entry, form)
            assert p["family"] == "tile" and p["tg"]["wn"] == wn, (name, p)
            assert p["tg"]["ntiles_n"] == (2 if nout > 160 else 1) and p["tg"]["ncols"] * p["tg"]["ntiles_n"] >= nout
    assert sorted(set(P.COL_NOUT.values())) == [1, 2, 3, 4, 5]
    assert [P.conv3t_geometry(1, 3, 5, n)["ncols"] % 32 for n in (36, 68, 100, 132, 164)] == [4, 4, 4, 4, 20]
    for nout in (60, 64, 68):
        assert P.plan_of(f"wcol-fwd-{nout}", "wino", "fwd", ("plain", True))["family"] == "wino"
        assert P.plan_of(f"wcol-bwd-{nout}", "wino", "bwd_data", ("identity", 0, False))["family"] == "wino"
    assert [P.cdiv(n, P.WINO_NT) for n in (60, 64, 68)] == [1, 1, 2]


def test_f4_cases():
    for name in P.F4_CASES:
        n, h, w, cin, cout = P.shape_of(name)
        setting = [s for s in P.settings_of(name) if s.startswith("wino4")][0]
        p = P.plan_of(name, setting, "fwd", ("plain", True)) if name not in P.SAVED else P.fwd_plan(P.SETTINGS[setting], n, h, w, cin, cin, cout)
        assert p["family"] == "wino4" and p["rows"] == n * p["g4"]["tiles_h"] * p["g4"]["tiles_w"] <= P.fwd_table_rows(n, h, w, cin, cout), name
        if "bwd_data" in P.CASES[name]["entries"]:
            assert P.plan_of(name, setting, "bwd_data", ("identity", 0, False))["family"] == "wino4", name
    g = P.wino4_geometry(*P.shape_of("f4-trtc")[1:3])
    assert g["tr"] != g["tc"] and g["tiles_h"] * g["tiles_w"] == 1
    g = P.wino4_geometry(*P.shape_of("f4-two-blocks")[1:3])
    assert g["tiles_w"] == 2 and g["tiles_h"] == 1 and 0 < P.shape_of("f4-two-blocks")[2] - 4 * g["tc"] < 4 * g["tc"]
    assert P.shape_of("f4-cred48")[3] == 48 and P.shape_of("f4-5x5")[3] == 16
    assert [P.cdiv(n, P.W4_NT) for n in (28, 32, 36)] == [1, 1, 2]
    n, h, w, cin, cout = P.shape_of("f4-plain")
    assert h % 4 and w % 4 and cout % P.W4_NT and cin % P.W4_NT and set(P.settings_of("f4-plain")) == {"wino4", "wino4-plain"}
    # a reduction that is no multiple of 16 is not taken
    assert P.wino4_fits(5, 5, 24, 32) is None and P.wino4_fits(5, 5, 32, 24) is not None


def test_implicit_gemm_and_narrow_cases():
    assert P.plan_of("gemm-cin12", "default", "fwd", ("plain", True))["family"] == "gemm"
    assert P.plan_of("gemm-cout12", "default", "bwd_data", ("identity", 0, False))["family"] == "gemm"
    for acc in (0, 1):
        assert P.plan_of("gemm-bnview", "default", "bwd_data", (O.ACT_RELU6, acc, False))["family"] == "gemm"
        assert (O.ACT_RELU6, acc, False) in P.forms_of("gemm-bnview", "bwd_data")
    assert P.plan_of("gemm-bnview", "default", "bwd_data", ("identity", 0, False))["family"] == "tile"
    n, h, w = P.shape_of("gemm-straddle")[:3]
    assert n == 3 and h * w == 35 and 128 % 35 and n * h * w < 128         # one 128-row tile holds all three images
    for name in ("narrow-16x4", "narrow-32x8"):
        for entry, form in (("fwd", ("plain", True)), ("bwd_data", ("identity", 0, False)), ("bwd_data_bn", (O.ACT_RELU6, "identity")), ("bwd_weight", ("plain", "identity"))):
            assert P.plan_of(name, "default", entry, form)["family"] == "narrow"
            assert P.plan_of(name, "gemm", entry, form)["family"] in ("gemm", "nine")
    assert P.shape_of("narrow-16x4")[3] == 4 * P.shape_of("narrow-16x4")[4]
    assert P.plan_of("not-narrow-24x8", "default", "fwd", ("plain", True))["family"] == "tile"
    for name in P.CASES:
        if name.startswith("direct-"):
            n, h, w = P.shape_of(name)[:3]
            for form in P.forms_of(name, "bwd_data_bn"):
                assert P.plan_of(name, "default", "bwd_data_bn", form)["family"] == "narrow-direct"
                assert P.plan_of(name, "no-direct", "bwd_data_bn", form)["family"] == "narrow"
    # pixels per wave and trip: a wave takes x0, x0 + 4, x0 + 8, x0 + 12 -- widths below, at and over 4 and 16
    assert sorted({P.shape_of(nm)[2] for nm in P.CASES if nm.startswith("direct-") and nm != "direct-2050rows"}) == [1, 3, 4, 5, 16, 17]
    n, h, w = P.shape_of("direct-2050rows")[:3]
    assert P.direct_blocks(n, h) == P.C3N_MAX_BLOCKS < n * h <= 2 * P.C3N_MAX_BLOCKS


def test_split_k_cases():
    """conv3_wgrad_splits: never an empty split, never fewer than the minimum while more than one; the named edges at 256 CUs"""
    for cus in CU_COUNTS:
        for name, case in P.CASES.items():
            if "bwd_weight" not in case["entries"]:
                continue
            for setting in case["settings"]:
                for form in P.forms_of(name, "bwd_weight"):
                    p = P.plan_of(name, setting, "bwd_weight", form, cus)
                    if "splits" in p:
                        assert (p["splits"] - 1) * p["sps"] < p["steps"] <= p["splits"] * p["sps"] and 0 < p["last"] <= p["sps"], (name, cus, p)
                        assert p["splits"] == 1 or p["sps"] >= (4 if p["family"] == "tile" else 8)
    plain = ("plain", "identity")
    p = P.plan_of("wgt-steps3", "default", "bwd_weight", plain)
    assert p["family"] == "tile" and p["steps"] == 3 and p["splits"] == 1
    p = P.plan_of("wgt-uneven", "default", "bwd_weight", plain)
    assert p["family"] == "tile" and (p["steps"], p["splits"], p["sps"], p["last"]) == (9, 2, 5, 4)
    assert P.ldx_of("wgt-pitch") == P.shape_of("wgt-pitch")[3] + 8
    tiles = set()
    for name in P.CASES:
        if name.startswith("wgt-") and "x" in name.split("-")[1]:
            n, h, w, cin, cout = P.shape_of(name)
            p = P.plan_of(name, "default", "bwd_weight", plain)
            assert p["family"] == "tile" and p["gx"] == P.cdiv(cin, 64) * P.cdiv(cout, 64) and p["steps"] == n * h * P.cdiv(w, 32)
            tiles.add((cin, cout, w))
    assert {w for _, _, w in tiles} == {1, 31, 32, 33} and {c for c, _, _ in tiles} == {4, 64, 68}
    bn = (O.ACT_RELU6, O.ACT_RELU6)
    steps, kinds = set(), set()
    for name in P.CASES:
        if name.startswith("nine-"):
            n, h, w, cin, cout = P.shape_of(name)
            p = P.plan_of(name, "default", "bwd_weight", bn)
            assert p["family"] == "nine" and p["nine"] == (12 if cout > 32 else 1) and p["steps"] == h * P.cdiv(w, 32)
            q = P.plan_of(name, "nine", "bwd_weight", plain)
            assert q["family"] == "nine" and q["nine"] == (4 if cout > 32 else 1)
            steps.add(p["steps"])
            kinds.update((p["nine"], q["nine"]))
            if p["steps"] == 17:
                assert (p["splits"], p["sps"], p["last"]) == (2, 9, 8)
            else:
                assert p["splits"] == 1
    assert steps == {7, 8, 17} and kinds == {12, 4, 1}
    for name in ("taps-36x36", "taps-4x132"):
        assert P.plan_of(name, "taps", "bwd_weight", bn)["family"] == P.plan_of(name, "taps", "bwd_weight", plain)["family"] == "taps"


def test_winograd_weight_gradient_cases():
    """the even deal: every unit of patches x steps is owned by exactly one block and no slot is left out, at three CU counts; the named
    edges at 256"""
    for cus in CU_COUNTS:
        for name in P.CASES:
            if name.startswith("ww-"):
                d = P.wino_wgrad_deal(cus, *P.shape_of(name))
                assert d["full"] * d["span"] + d["tail"] == d["steps"] and 0 <= d["tail"] < d["span"] <= d["steps"]
                assert d["span"] >= min(4, d["steps"])
                assert d["full"] * d["patches"] * d["span"] + sum(min(d["span"], d["patches"] * d["tail"] - i * d["span"]) for i in range(len(d["walks"]))) == \
                    d["patches"] * d["steps"]
                # the slots of a patch: its full chunks and every tail block that touches it
                if d["tail"]:
                    for patch in range(d["patches"]):
                        first, last = patch * d["tail"] // d["span"], ((patch + 1) * d["tail"] - 1) // d["span"]
                        assert d["full"] + last - first + 1 <= d["slots"]
    plain = ("plain", "identity")
    deal = lambda name: P.plan_of(name, "wino", "bwd_weight", plain)      # noqa: E731
    for name in P.CASES:
        if name.startswith("ww-"):
            n, h, w = P.shape_of(name)[:3]
            assert deal(name)["family"] == "wino" and h % 2 == 0 and w % 2 == 0, name
    assert [deal(f"ww-w{w}")["wrem"] for w in (2, 30, 32, 34)] == [2, 30, 32, 2] and P.shape_of("ww-w2")[1] == 2
    assert [deal(f"ww-{c}")["patches"] for c in ("4x4", "64x64", "132x64", "4x132")] == [1, 1, 3, 3]
    d = deal("ww-span-is-steps")
    assert d["steps"] == 2 == d["span"] and d["tail"] == 0
    d = deal("ww-span-floor")
    assert d["span"] == 4 and P.cdiv(d["patches"] * d["steps"], P.NUM_CUS) < 4 <= d["steps"]
    d = deal("ww-tail-two")
    assert (d["span"], d["full"], d["tail"]) == (4, 1, 2) and d["walks"] == [2, 2]
    d = deal("ww-tail-three")
    assert (d["span"], d["tail"]) == (5, 2) and max(d["walks"]) == 3
    d = deal("ww-5x4x32")
    assert (d["steps"], d["span"], d["full"], d["tail"], len(d["walks"])) == (10, 4, 2, 2, 3)
    d = deal("ww-9x2x32")
    assert (d["steps"], d["tail"]) == (9, 1) and d["walks"] == [4, 2]
    # odd sizes are declined
    assert P.plan_of("px-9x33", "wino", "bwd_weight", plain)["family"] == "tile"


def test_saved_pair_cases():
    for name, (setting, shape) in P.SAVED.items():
        env = P.SETTINGS[setting]
        assert P.saved_pair(env, *shape) and P.saved_floats(env, *shape) == shape[0] * (shape[1] + 2) * (shape[2] + 2) * shape[3]
        assert P.fwd_plan(env, *shape[:3], shape[3], *shape[3:])["family"] == setting
        assert P.ldx_of(name) > shape[3] and P.c_froms(name) == (0, 4, shape[3] - 4)
        assert not P.saved_pair(dict(env, SSDSEG_CONV3_SAVED="0"), *shape) and not P.saved_pair(dict(env, SSDSEG_CONV3_WGRAD="nine"), *shape)
    assert not P.saved_pair({}, 2, 4, 6, 16, 32) and not P.saved_pair(P.SETTINGS["wino"], 2, 5, 6, 16, 32)
    k = P.lattice_case("saved-f2")
    before, want = P.saved_copy(k, O.ACT_RELU6, 4)
    assert np.isnan(before[..., 4:]).all() and np.array_equal(before[..., :4], want[..., :4])
    assert not want[:, 0].any() and not want[:, -1].any() and not want[:, :, 0].any() and not want[:, :, -1].any() and want[:, 1:-1, 1:-1].any()


# ------------------------------------------------------------------------------------------------------- the F(4x4) bound
def _ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("name", P.F4_CASES)
def test_f4_emulation_stays_within_the_bound_and_a_wrong_weight_does_not(name):
    """float32 NumPy emulation of U = G w G^T, V = B^T d B, sum_c U . V and A^T [.] A: inside the per-position bound on the lattice and
    the normal data of every F(4x4) shape, and not below 0.01 of it overall (test_f4_bound_is_not_slack); with the centre tap of the
    most active input channel off by 2^-10 relative it is outside on the normal data of every shape, and at 0.7 of it or more on
    the lattice data: the bound cannot hide a wrong constant"""
    for k in (P.lattice_case(name), P.normal_case(name)):
        for view in ("plain", O.ACT_RELU6):
            y, b = P.ref_fwd(k, view)[0], P.f4_bound_fwd(k, view)
            assert (b > 0).all() and (b <= P.f4_bound_issue(P.view_abs(k, view), k.w.astype(np.float64), k.shape[3]) * (1 + 1e-9)).all()
            assert _ratio(P.f4_emulation(k, view), y, b) <= 1.0, (name, k.mode, view)
            kept = k.w
            try:
                c = int((np.abs(P.in_view(k, view)[0]).sum(axis=(0, 1, 2)) * np.abs(kept[1, 1]).sum(axis=1)).argmax())
                k.w = kept.copy()
                k.w[1, 1, c, :] *= F32(1 + 2.0 ** -10)
                # (the lattice's weights are smaller against its data: measured 0.73 at 48 channels, above 1 on most shapes -- held
                # there so that a slacker bound shows)
                assert _ratio(P.f4_emulation(k, view), y, b) > (1.0 if k.mode == "normal" else 0.7), (name, k.mode, view)
            finally:
                k.w = kept


def test_f4_bound_is_not_slack():
    worst = max(_ratio(P.f4_emulation(k, view), P.ref_fwd(k, view)[0], P.f4_bound_fwd(k, view))
                for k in (P.normal_case(name) for name in P.NORMAL_CASES if name in P.F4_CASES) for view in ("plain", O.ACT_RELU6))
    assert 0.01 <= worst <= 1.0, worst
    assert P.F4_ROUNDINGS == 19


def test_normal_bounds_are_positive_and_small():
    for name in P.NORMAL_CASES:
        k = P.normal_case(name)
        z = k.x.astype(np.float64) * k.scale + k.shift
        zg = k.yraw.astype(np.float64) * k.gscale + k.gshift
        for pre in (z, zg):
            assert np.minimum(np.abs(pre), np.abs(pre - 6)).min() >= P.BAND * 0.99
        b = P.normal_bounds(k, O.ACT_RELU6, O.ACT_RELU6, 1)
        y = P.ref_fwd(k, O.ACT_RELU6)[0]
        for q, ref in (("y", y), ("dx", P.ref_dx(k, O.ACT_RELU6, 1)), ("dW", P.ref_dw(k, O.ACT_RELU6, O.ACT_RELU6))):
            assert (b[q] > 0).all() and b[q].max() < 1e-2 * max(np.abs(ref).max(), 1.0), (name, q)
        assert (P.sumsq_bound(y, b["y"]) < 5e-2 * (y * y).sum(axis=(0, 1, 2)) + 1e-6).all()
