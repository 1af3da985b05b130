"""Named edge cases, the float64 reference, bounds and a mirror of the host geometry for the dense 3x3 conv kernels: plain NumPy.

The entry points are ssdseg_conv3x3_parts / _saved_floats / _fwd / _fwd_saved / _fwd_saved_from / _bwd_weight_saved / _bwd_data /
_bwd_data_bn / _bwd_weight (csrc/conv3.hip with conv3_tile.h, conv3_wino.h, conv3_wino4.h, conv3_wgrad.h, conv3_wgrad_tile.h,
conv3_wino_wgrad.h; csrc/conv3n.hip; the implicit-GEMM paths of csrc/gemm.hip).  tests/test_cpu_conv3_cases.py vets the reference, the
cases and the mirror on the CPU; tests/test_gpu_conv3_edges.py runs the kernels on the same cases.  Every builder seeds its own
generator from the case's name, so the same call gives the same arrays in both files.  Shapes are (n, h, w, cin, cout).

The lattice family.  x, g, yraw, the shifts, k1, k0 and mean are multiples of 1/4 (`fine`) or integers (`coarse`), the weights multiples
of 1/8 (1/2), scales and invstd signed powers of two, so every product and every sum the kernels form is a float32 number in any order, fused or not: the float64 reference IS the float32 result and the bound is 0.
`budget` gives, in units of each result's lattice, the sum of the absolute terms of every reduction; below 2^24 no partial sum leaves
the integers float32 holds exactly.  That includes the transformed domains of Winograd F(2x2, 3x3), whose matrices hold only 0, +-1
and 1/2: V = B^T d B and Z = A dY A^T stay on the data's lattice, U = G w G^T is a quarter of the weights' lattice (two halvings),
sum_c U.V and A^T [.] A are sums on the product lattice, and the weight gradient G^T [sum_tiles V.Z] G halves twice after the sums --
every one of them is budgeted with the absolute matrices, so the partial-slab sums (any subset of the tiles) are covered too.  The
(scale, shift) pairs put many pre-activations exactly on 0 and exactly on 6 in both views: nothing is nudged.

The normal family.  N(0, 2) data off the lattice, pre-activations kept out of a 1e-4 band around 0 and 6, any-order bounds
(U = 2^-24, gamma(L) = L U / (1 - L U)); the derivations stand in the docstring of tests/test_gpu_conv3_edges.py.

F(4x4, 3x3) is exact in neither family (G holds 1/6, 1/12, 1/24; B^T and A^T constants up to 8): `f4_bound` (docstring there).

The mirror is of the GEOMETRY the cases are named after: conv3t_geometry, wino4_geometry / wino4_fits, conv3_wgrad_splits with the
step definitions of the halo-tile and nine-tap weight gradients, the even deal of the Winograd weight gradient, conv3_fwd_table_rows
(== ssdseg_conv3x3_parts), and the family each plan function picks (to know which kernel a setting is there for); the kernel symbols
of every shape and switch are pinned in tests/test_gpu_conv3_dispatch.py, not here.
"""
import functools
import re

import numpy as np

from oracle import np_ops as O
import _pw_cases as PW

F32 = np.float32
U = 2.0 ** -24
EXACT = 2 ** 24
gamma, cdiv = PW.gamma, PW.cdiv
ACT_NAMES = PW.ACT_NAMES
NUM_CUS = 256                   # the MI355X; the GPU file passes the device's own count
# every switch the dense 3x3 conv reads per call, and (its narrow and implicit-GEMM forms run pointwise GEMMs) the pointwise ones
CONV3_VARS = ("SSDSEG_CONV3_NARROW", "SSDSEG_CONV3_TILE", "SSDSEG_CONV3_WINOGRAD", "SSDSEG_CONV3_F4", "SSDSEG_CONV3_WGRAD", "SSDSEG_CONV3_SAVED",
              "SSDSEG_CONV3N_DIRECT", "SSDSEG_W4_GROUP", "SSDSEG_W4_BLOCKS", "SSDSEG_W4_PLAIN_STORES", "SSDSEG_W4_TRACE") + PW.PW_VARS
SETTINGS = {
    "default": {},
    "wino": {"SSDSEG_CONV3_WINOGRAD": "1", "SSDSEG_CONV3_F4": "0"},
    "wino4": {"SSDSEG_CONV3_WINOGRAD": "1", "SSDSEG_CONV3_F4": "1"},
    "wino4-plain": {"SSDSEG_CONV3_WINOGRAD": "1", "SSDSEG_CONV3_F4": "1", "SSDSEG_W4_PLAIN_STORES": "1"},
    "gemm": {"SSDSEG_CONV3_TILE": "0", "SSDSEG_CONV3_NARROW": "0"},
    "no-direct": {"SSDSEG_CONV3N_DIRECT": "0"},
    "nine": {"SSDSEG_CONV3_WGRAD": "nine"},
    "taps": {"SSDSEG_CONV3_WGRAD": "taps"},
}


def seeded(*key):
    return np.random.default_rng([1993, 303] + [int(k) for k in key])


# ================================================================================================= mirror of the host geometry
C3T_ROWS, C3T_COLS, C3T_KC = 8, 32, 8
WINO_NT, W4_NT, W4_THREADS, W4_RL, W4_QP_MAX = 64, 32, 256, 12, 1040
W3T_KT = W3T_NT = 64
W3T_COLS = C9_PX = C9_KT = 32
WWG_KT = WWG_NT = 64
C3N_MAX_COUT, C3N_CIN, C3N_MAX_BLOCKS = 8, 256, 2048
LDS_160K = 160 * 1024


def wino_lds_floats(cred):
    raw, u_f, ms, red = 2 * 344 * 4, 16 * WINO_NT * C3T_KC, 4 * 2 * 64 * 2 * 33, 2 * 2 * 8 * 32
    return max(2 * raw + 3 * u_f + 2 * (cred + 16), ms + red)


def wino4_lds_floats(cred):
    return 2 * (4 * W4_QP_MAX * 4) + 1024 + 2 * (cred + 16)


def conv3t_geometry(n, h, w, nout):
    tiles_h, tiles_w = cdiv(h, C3T_ROWS), cdiv(w, C3T_COLS)
    ntiles_n = cdiv(nout, 160)
    ncols = (cdiv(nout, ntiles_n) + 3) // 4 * 4
    return dict(tiles_h=tiles_h, tiles_w=tiles_w, mtiles=n * tiles_h * tiles_w, ntiles_n=ntiles_n, ncols=ncols, wn=cdiv(ncols, 32))


def wino4_geometry(h, w):
    best, g = -1, None
    for tc in range(1, 12):
        tr = 1
        while tr * tc <= 32:
            if 4 * tr * (4 * tc + 2) <= 2 * W4_THREADS:
                trs = 24 * W4_RL
                while (trs & 15) != (tc & 15):
                    trs += 1
                if tr * trs + 15 <= W4_QP_MAX:
                    blocks = cdiv(h, 4 * tr) * cdiv(w, 4 * tc)
                    key = blocks * 1024 + abs(tr - tc)
                    if best < 0 or key < best:
                        best, g = key, dict(tr=tr, tc=tc, trs=trs, tiles_h=cdiv(h, 4 * tr), tiles_w=cdiv(w, 4 * tc))
            tr += 1
    return g


def wino4_fits(h, w, cred, nout):
    if cred % 16 != 0 or wino_lds_floats(cred) * 4 > LDS_160K or wino4_lds_floats(cred) * 4 > LDS_160K:
        return None
    g = wino4_geometry(h, w)
    return g if g is not None and 36 * cred * cdiv(nout, W4_NT) * W4_NT * 4 < (1 << 31) else None


def switches(env):
    tile = env.get("SSDSEG_CONV3_TILE", "")[:1] != "0"
    wv = env.get("SSDSEG_CONV3_WINOGRAD")
    wino = 0 if (not tile or (wv or "")[:1] == "0") else (2 if not wv else 1)
    f4 = {"0": 0, "1": 1}.get(env.get("SSDSEG_CONV3_F4", "")[:1], 2)
    wg = env.get("SSDSEG_CONV3_WGRAD")
    wgrad = "unset" if wg is None else (wg if wg in ("taps", "nine") else "other")
    return dict(narrow=env.get("SSDSEG_CONV3_NARROW", "")[:1] != "0", tile=tile, wino=wino, f4=f4, wgrad=wgrad, saved="SSDSEG_CONV3_SAVED" not in env,
                direct=env.get("SSDSEG_CONV3N_DIRECT", "")[:1] != "0")


def is_narrow(sw, cin, cout):
    return sw["narrow"] and cout <= C3N_MAX_COUT and cin >= 4 * cout


def tile_fits(n, h, w, ld):
    return n * h * w * ld * 4 < (1 << 31)


def wino_takes(sw, n, h, w, cred, nout):
    if sw["wino"] == 0 or cred % C3T_KC != 0 or wino_lds_floats(cred) * 4 > LDS_160K:
        return False
    return sw["wino"] == 1 or (nout >= 64 and n * cdiv(h, C3T_ROWS) * cdiv(w, C3T_COLS) >= 256)


def wino4_takes(sw, n, h, w, cred, nout):
    g = wino4_fits(h, w, cred, nout) if sw["f4"] != 0 else None
    if g is None:
        return None
    return g if (sw["f4"] == 1 or n * g["tiles_h"] * g["tiles_w"] * cdiv(nout, W4_NT) >= 2048) else None


def tiled_plan(sw, n, h, w, ld, cred, nout):
    """conv3_tiled_plan -> None | dict(family, rows, tg, g4)"""
    if not sw["tile"] or cred % C3T_KC != 0 or not tile_fits(n, h, w, ld):
        return None
    tg = conv3t_geometry(n, h, w, nout)
    p = dict(family="tile", rows=tg["mtiles"], tg=tg, g4=None)
    if wino_takes(sw, n, h, w, cred, nout):
        g4 = wino4_takes(sw, n, h, w, cred, nout)
        if g4 is None:
            p["family"] = "wino"
        else:
            p.update(family="wino4", g4=g4, rows=n * g4["tiles_h"] * g4["tiles_w"])
    return p


def gemm_rows(n, h, w, cout):
    return PW.rowA_grid_y(n * h * w, cout, {})


def fwd_plan(env, n, h, w, ldx, cin, cout):
    sw = switches(env)
    if is_narrow(sw, cin, cout):
        return dict(family="narrow", rows=gemm_rows(n, h, w, cout))
    return tiled_plan(sw, n, h, w, ldx, cin, cout) or dict(family="gemm", rows=gemm_rows(n, h, w, cout))


def fwd_table_rows(n, h, w, cin, cout):
    """conv3_fwd_table_rows == ssdseg_conv3x3_parts: the largest row count among the forward kernels that can take the layer"""
    rows = gemm_rows(n, h, w, cout)
    if cin % C3T_KC != 0:
        return rows
    rows = max(rows, conv3t_geometry(n, h, w, cout)["mtiles"])
    g = wino4_fits(h, w, cin, cout)
    return max(rows, n * g["tiles_h"] * g["tiles_w"]) if g else rows


def bwd_data_plan(env, n, h, w, ldx, cin, cout, gview_bn, in_bn):
    sw = switches(env)
    if is_narrow(sw, cin, cout):
        direct = in_bn and sw["direct"] and cin == C3N_CIN and cout == 4 and ldx % 4 == 0 and n * h * w < (1 << 29)
        return dict(family="narrow-direct" if direct else "narrow")
    p = None if gview_bn else tiled_plan(sw, n, h, w, cout, cout, cin)
    return p or dict(family="gemm")


def wgrad_splits(steps, want, min_steps):
    """conv3_wgrad_splits -> (splits, steps per split): as many as wanted while each keeps min_steps, dealt evenly (no empty split)"""
    splits = max(min(want, steps // min_steps), 1)
    sps = cdiv(steps, splits)
    return cdiv(steps, sps), sps


def wino_wgrad_takes(sw, n, h, w, cin, cout):
    if sw["wino"] == 0 or h % 2 or w % 2 or n * (h + 2) * (w + 2) * cin * 4 >= (1 << 31) or n * h * w * cout * 4 >= (1 << 31):
        return False
    return sw["wino"] == 1 or n * (h // 2) * cdiv(w, 32) >= 512


def wgrad_family(sw, n, h, w, ldx, cin, cout, gview_bn):
    plain = sw["wgrad"] == "unset" and not gview_bn
    if is_narrow(sw, cin, cout):
        return "narrow"
    if plain and wino_wgrad_takes(sw, n, h, w, cin, cout):
        return "wino"
    if plain and sw["tile"] and tile_fits(n, h, w, ldx) and tile_fits(n, h, w, cout):
        return "tile"
    return "nine" if sw["wgrad"] != "taps" else "taps"


def wino_wgrad_deal(num_cus, n, h, w, cin, cout):
    """the even deal of conv3_wino_wgrad_launch -> dict(steps, strips, wrem, patches, span, full, tail, slots, blocks, walks: patches
    each tail block works on in turn)"""
    strips = cdiv(w, 32)
    steps = n * (h // 2) * strips
    patches = cdiv(cin, WWG_KT) * cdiv(cout, WWG_NT)
    span = min(max(cdiv(patches * steps, num_cus), 4), steps)
    full = steps // span
    tail = steps - full * span
    slots = full + ((cdiv(tail, span) + 1) if tail > 0 else 0)
    tail_blocks = cdiv(patches * tail, span)
    walks = []
    for tb in range(tail_blocks):
        u, uend = tb * span, min(tb * span + span, patches * tail)
        walks.append(len({v // tail for v in range(u, uend)}))
    return dict(steps=steps, strips=strips, wrem=w - 32 * (strips - 1), patches=patches, span=span, full=full, tail=tail, slots=slots,
                blocks=full * patches + tail_blocks, walks=walks)


def wgrad_plan(env, num_cus, n, h, w, ldx, cin, cout, gview_bn):
    sw = switches(env)
    p = dict(family=wgrad_family(sw, n, h, w, ldx, cin, cout, gview_bn))
    if p["family"] == "tile":
        p["gx"] = cdiv(cin, W3T_KT) * cdiv(cout, W3T_NT)
        p["steps"] = n * cdiv(w, W3T_COLS) * h
        p["splits"], p["sps"] = wgrad_splits(p["steps"], 2 * num_cus // p["gx"], 4)
    elif p["family"] == "nine":
        wn = 4 if cout > 32 else 1
        p["nine"] = 12 if (wn == 4 and sw["wgrad"] != "nine") else wn
        p["gx"], p["gy"] = cdiv(cout, 32 * wn), cdiv(cin, C9_KT)
        p["steps"] = n * h * cdiv(w, C9_PX)
        p["splits"], p["sps"] = wgrad_splits(p["steps"], 2 * num_cus // (p["gx"] * p["gy"]), 8)
    elif p["family"] == "wino":
        p.update(wino_wgrad_deal(num_cus, n, h, w, cin, cout))
    if "splits" in p:
        p["last"] = p["steps"] - (p["splits"] - 1) * p["sps"]
    return p


def saved_pair(env, n, h, w, cin, cout):
    sw = switches(env)
    return sw["saved"] and fwd_plan(env, n, h, w, cin, cin, cout)["family"] in ("wino", "wino4") and \
        wgrad_family(sw, n, h, w, cin, cin, cout, False) == "wino"


def saved_floats(env, n, h, w, cin, cout):
    return n * (h + 2) * (w + 2) * cin if saved_pair(env, n, h, w, cin, cout) else 0


def direct_blocks(n, h):
    return min(n * h, C3N_MAX_BLOCKS)


def kernel_for(entry, plan, with_view=False):
    """a regular expression of the kernel symbol (timing registry spelling) the plan's family runs"""
    fam = plan["family"]
    role = "fwd" if entry in ("fwd", "saved") else "bwd_data"
    tf = "true" if with_view else "false"
    if entry == "bwd_weight":
        return {"narrow": r"^conv3n_shift_kernel$", "wino": r"^conv3_wino_wgrad_kernel$", "tile": r"^conv3_wgrad_tile_kernel$",
                "taps": r"^gemm_wgrad_kernel<.*\[conv3x3 tap\]$",
                "nine": r"conv3_wgrad12_kernel" if plan.get("nine") == 12 else r"conv3_wgrad9_kernel<%d>" % plan.get("nine", 0)}[fam]
    return {"narrow": r"^conv3n_tapsum_kernel$" if role == "fwd" else r"^conv3n_shift_kernel$", "narrow-direct": r"^conv3n_bwd_bn_direct_kernel$",
            "tile": r"^conv3_tile_kernel<%d> \[%s\]$" % (plan["tg"]["wn"] if "tg" in plan else 0, role),
            "wino": r"^conv3_wino_kernel<%s> \[%s\]$" % (tf, role), "wino4": r"^conv3_wino4_kernel<%s> \[%s\]$" % (tf, role),
            "gemm": r"^gemm_rowA_kernel<\d, %d, 1, " % (0 if role == "fwd" else 1)}[fam]


def reaches(launches, pattern):
    return any(re.search(pattern, s) for s in launches)


# ============================================================================================================ the cases
# name: dict(shape, settings, entries, ldx (row pitch of x and dx) or None, why)
CASES = {}
ALL_ENTRIES = ("fwd", "bwd_data", "bwd_data_bn", "bwd_weight")


def _case(name, shape, settings, entries=ALL_ENTRIES, why="", ldx=None):
    assert name not in CASES, name
    CASES[name] = dict(shape=tuple(shape), settings=tuple(settings), entries=tuple(entries), ldx=ldx, why=why)


# ---- pixel tiles of the halo-tile and F(2x2) kernels, both roles
_case("px-1x1", (1, 1, 1, 8, 8), ("default", "wino"), why="one pixel")
_case("px-8x32", (1, 8, 32, 16, 16), ("default", "wino"), why="one whole 8 x 32 tile")
_case("px-9x33", (2, 9, 33, 16, 16), ("default", "wino"), why="ragged tile row and column; halos meet the other image's rows")
_case("px-7x31", (2, 7, 31, 16, 16), ("default", "wino"), why="one short of the tile; odd h and w: a partial 2 x 2 tile")
# ---- column tiles of conv3_tile_kernel<WN>: forward through cout, input gradient through cin; F(2x2) around its 64-column tile
COL_NOUT = {32: 1, 36: 2, 68: 3, 96: 3, 100: 4, 132: 5, 160: 5, 164: 3, 168: 3}       # nout: WN
for _nout in COL_NOUT:
    _case(f"col-fwd-{_nout}", (1, 3, 5, 8, _nout), ("default",), ("fwd",), why="column tiles, forward role")
    _case(f"col-bwd-{_nout}", (1, 3, 5, _nout, 16), ("default",), ("bwd_data", "bwd_data_bn"), why="column tiles, input-gradient role")
for _nout in (60, 64, 68):
    _case(f"wcol-fwd-{_nout}", (1, 4, 6, 8, _nout), ("wino",), ("fwd",), why="F(2x2) column tile")
    _case(f"wcol-bwd-{_nout}", (1, 4, 6, _nout, 16), ("wino",), ("bwd_data",), why="F(2x2) column tile, input-gradient role")
# ---- F(4x4): below, at and one over a 4 x 4 tile both ways; block geometry; reduction steps; column tiles; plain stores
for _h in (1, 2, 3, 4, 5):
    for _w in (1, 2, 3, 4, 5):
        _case(f"f4-{_h}x{_w}", (2, _h, _w, 16, 32), ("wino4",), ("fwd", "bwd_data"), why="F(4x4) tile edge")
_case("f4-trtc", (1, 4, 40, 16, 32), ("wino4",), ("fwd", "bwd_data"), why="tr != tc")
_case("f4-two-blocks", (1, 4, 50, 16, 32), ("wino4",), ("fwd", "bwd_data"), why="two blocks along w, the last partial")
_case("f4-cred48", (2, 5, 6, 48, 32), ("wino4",), ("fwd",), why="three 16-channel steps")
for _nout in (28, 32, 36):
    _case(f"f4-nout{_nout}", (1, 5, 6, 16, _nout), ("wino4",), ("fwd",), why="F(4x4) 32-column tile")
_case("f4-plain", (2, 5, 7, 16, 48), ("wino4", "wino4-plain"), ("fwd", "bwd_data"), why="SSDSEG_W4_PLAIN_STORES on a ragged shape")
# ---- implicit GEMM
_case("gemm-cin12", (1, 6, 8, 12, 16), ("default", "gemm"), ("fwd", "bwd_weight"), why="cin % 8 != 0: forward")
_case("gemm-cout12", (1, 6, 8, 16, 12), ("default", "gemm"), ("bwd_data", "bwd_data_bn"), why="cout % 8 != 0: input gradient")
_case("gemm-bnview", (2, 5, 7, 16, 16), ("default", "gemm"), ("bwd_data", "bwd_data_bn"), why="BatchNorm gradient view, accumulate 0 and 1")
_case("gemm-straddle", (3, 5, 7, 12, 12), ("default", "gemm"), why="n = 3, h w = 35: 128-row tiles straddle the image borders")
# ---- narrow
_case("narrow-16x4", (2, 5, 6, 16, 4), ("default", "gemm"), why="cin == 4 cout exactly")
_case("narrow-32x8", (1, 5, 5, 32, 8), ("default", "gemm"), why="narrow, cout 8")
_case("not-narrow-24x8", (1, 5, 5, 24, 8), ("default",), why="cin < 4 cout: not narrow")
for _h in (1, 2):
    for _w in (1, 3, 4, 5, 16, 17):
        _case(f"direct-{_h}x{_w}", (2, _h, _w, 256, 4), ("default", "no-direct"), ("bwd_data_bn",), why="the direct kernel's pixel trips")
_case("direct-2050rows", (1025, 2, 1, 256, 4), ("default", "no-direct"), ("bwd_data_bn",), why="2,050 image rows on 2,048 blocks: a block walks two")
# ---- weight gradient, halo tile (identity gradient view, default switches)
for _cin, _cout in ((4, 4), (64, 64), (68, 68), (4, 68), (68, 64)):
    for _w in ((1, 31, 32, 33) if _cin == _cout else (33,)):
        _case(f"wgt-{_cin}x{_cout}-w{_w}", (2, 4, _w, _cin, _cout), ("default",), ("bwd_weight",), why="halo-tile weight gradient: channel tiles, strips")
_case("wgt-steps3", (1, 3, 5, 16, 16), ("default",), ("bwd_weight",), why="3 steps < 4: one split, copied straight to dW")
_case("wgt-uneven", (1, 9, 5, 16, 16), ("default",), ("bwd_weight",), why="9 steps dealt 5 + 4: a shorter last split")
_case("wgt-pitch", (2, 5, 33, 16, 16), ("default",), ("bwd_weight",), why="ldx = cin + 8, NaN outside the slice", ldx=24)
# ---- weight gradient, nine taps in one pass (BatchNorm gradient view; identity under a setting) and a GEMM per tap
NINE_GEO = ((7, 1), (8, 32), (17, 32), (4, 33))          # (h, w) at n = 1: 7, 8, 17 and 8 steps
for _i, (_cin, _cout) in enumerate(((4, 4), (32, 32), (36, 36), (4, 132), (36, 132), (32, 36))):
    for _h, _w in NINE_GEO:
        _case(f"nine-{_cin}x{_cout}-{_h}x{_w}", (1, _h, _w, _cin, _cout), ("default", "nine"), ("bwd_weight",), why="nine-tap weight gradient")
_case("taps-36x36", (1, 8, 32, 36, 36), ("taps",), ("bwd_weight",), why="a GEMM per tap")
_case("taps-4x132", (1, 4, 33, 4, 132), ("taps",), ("bwd_weight",), why="a GEMM per tap")
# ---- weight gradient, Winograd (forced; identity gradient view)
for _w in (2, 30, 32, 34):
    _case(f"ww-w{_w}", (3, 2, _w, 68, 68), ("wino",), ("bwd_weight",), why="wrem 2, 30, 32, 2; h = 2")
for _cin, _cout in ((4, 4), (64, 64), (132, 64), (4, 132)):
    _case(f"ww-{_cin}x{_cout}", (2, 4, 32, _cin, _cout), ("wino",), ("bwd_weight",), why="channel patches")
_case("ww-span-is-steps", (1, 2, 34, 64, 64), ("wino",), ("bwd_weight",), why="2 steps < 4: span = steps")
_case("ww-span-floor", (4, 2, 32, 64, 64), ("wino",), ("bwd_weight",), why="span held at its floor of 4")
_case("ww-tail-two", (3, 4, 32, 68, 68), ("wino",), ("bwd_weight",), why="6 steps: tail 2, tail blocks walk two patches")
_case("ww-tail-three", (172, 2, 2, 132, 68), ("wino",), ("bwd_weight",), why="172 steps x 6 patches: span 5, tail 2, a tail block walks three patches")
_case("ww-5x4x32", (5, 4, 32, 132, 72), ("wino",), ("bwd_weight",), why="10 steps: 2 full chunks of 4 + a 2-step tail")
_case("ww-9x2x32", (9, 2, 32, 72, 136), ("wino",), ("bwd_weight",), why="9 steps: a 1-step tail, a tail block walks four patches")
# ---- the saved-input pair
SAVED = {"saved-f2": ("wino", (2, 4, 6, 16, 32)), "saved-f4": ("wino4", (2, 4, 6, 16, 32)), "saved-f2-w34": ("wino", (1, 2, 34, 24, 64))}
for _name, (_setting, _shape) in SAVED.items():
    _case(_name, _shape, (_setting,), (), why="ssdseg_conv3x3_fwd_saved_from / _bwd_weight_saved", ldx=_shape[3] + 8)


def shape_of(name):
    return CASES[name]["shape"]


def settings_of(name):
    return CASES[name]["settings"]


def ldx_of(name):
    return CASES[name]["ldx"] or shape_of(name)[3]


def c_froms(name):
    cin = shape_of(name)[3]
    return (0, 4, cin - 4)


# ------------------------------------------------------------------------------------------------------------ the forms
# A view is "plain" | "identity" or the activation code of an affine / BatchNorm-backward view.
# forward: (input view, stats); input gradient: (gradient view, accumulate, into a channel slice); fused BatchNorm: (input view,
# gradient view); weight gradient: (input view, gradient view)
FWD_FORMS = [("plain", True), (O.ACT_RELU6, True), (O.ACT_RELU, False), (O.ACT_NONE, True), (O.ACT_ZERO, True)]
DATA_FORMS = [("identity", 0, False), ("identity", 1, False), ("identity", 0, True), ("identity", 1, True), (O.ACT_RELU6, 0, False),
              (O.ACT_RELU6, 1, False), (O.ACT_RELU, 0, True)]
BN_FORMS = [(O.ACT_RELU6, "identity"), (O.ACT_RELU6, O.ACT_RELU6), (O.ACT_RELU, "identity"), (O.ACT_NONE, O.ACT_RELU)]
WEIGHT_FORMS = [("plain", "identity"), (O.ACT_RELU6, "identity"), (O.ACT_RELU6, O.ACT_RELU6), (O.ACT_NONE, O.ACT_RELU), (O.ACT_RELU, O.ACT_ZERO)]
FORMS = dict(fwd=FWD_FORMS, bwd_data=DATA_FORMS, bwd_data_bn=BN_FORMS, bwd_weight=WEIGHT_FORMS)
BIG = 200000      # pixels x channels from which a case runs two forms per entry point only


def forms_of(name, entry):
    if entry not in CASES[name]["entries"]:
        return []
    n, h, w, cin, cout = shape_of(name)
    forms = FORMS[entry]
    return [forms[0], forms[2]] if n * h * w * max(cin, cout) >= BIG else forms


def form_name(form):
    return "+".join(ACT_NAMES.get(f, str(f)) if not isinstance(f, (bool, str)) else str(f) for f in form)


def plan_of(name, setting, entry, form, num_cus=NUM_CUS):
    """the plan (family and geometry) of one form of one entry point of a case under a setting"""
    n, h, w, cin, cout = shape_of(name)
    env, ldx = SETTINGS[setting], ldx_of(name)
    if entry == "fwd":
        return fwd_plan(env, n, h, w, ldx, cin, cout)
    if entry == "bwd_data":
        return bwd_data_plan(env, n, h, w, ldx, cin, cout, form[0] != "identity", False)
    if entry == "bwd_data_bn":
        return bwd_data_plan(env, n, h, w, ldx, cin, cout, form[1] != "identity", True)
    return wgrad_plan(env, num_cus, n, h, w, ldx, cin, cout, form[1] != "identity")


def expected_kernel(name, setting, entry, form, num_cus=NUM_CUS):
    with_view = entry == "fwd" and form[0] != "plain"
    return kernel_for(entry, plan_of(name, setting, entry, form, num_cus), with_view)


# ---------------------------------------------------------------------------------------------------- lattice inputs
PARAMS = PW.PARAMS      # (scale, shift) per channel, in turn: pre-activations on both thresholds, both signs of the scale
LATTICE = {   # mode: (denominator of x / g / yraw / shifts / k / mean, of the weights, largest numerator of x, of w)
    "fine": (4, 8, 8, 3),
    "coarse": (1, 2, 2, 2),
}
MODES = ("fine", "coarse")


class Case:
    pass


def _build(name, mode):
    n, h, w, cin, cout = shape_of(name)
    xd, wd, xmax, wmax = LATTICE[mode]
    rng = seeded(*[ord(ch) for ch in name])
    k = Case()
    k.name, k.shape, k.mode, k.xd, k.wd, k.ldx = name, (n, h, w, cin, cout), mode, xd, wd, ldx_of(name)

    def grid(shape, top, den):
        return (rng.integers(-top, top + 1, shape) / den).astype(F32)

    gmax = max(xmax // 2, 1)
    k.x = grid((n, h, w, cin), xmax, xd)
    k.w = grid((3, 3, cin, cout), wmax, wd)
    k.g = grid((n, h, w, cout), gmax, xd)
    k.yraw = grid((n, h, w, cout), xmax, xd)
    k.base = grid((n, h, w, cin), gmax, xd)
    # the corners of every image, the last channel and every tap carry non-zero terms
    for a in (k.x, k.g):
        a[:, 0, 0, -1] = a[:, -1, -1, -1] = a[:, 0, -1, 0] = a[:, -1, 0, 0] = F32(1)
    k.w[:, :, -1, -1] = k.w[:, :, 0, -1] = k.w[:, :, -1, 0] = F32(1.0 / wd)
    par = np.array(PARAMS, np.float64)
    ci, co = np.arange(cin), np.arange(cout)
    k.scale = par[(ci + 1) % 8, 0].astype(F32)
    k.shift = par[(ci + 1) % 8, 1].astype(F32)
    k.gscale = par[(co * 3 + 2) % 8, 0].astype(F32)
    k.gshift = par[(co * 3 + 2) % 8, 1].astype(F32)
    k.k1 = (((co * 5) % 3 - 1) / xd).astype(F32)
    k.k0 = (((co * 7) % 5 - 2) / xd).astype(F32)
    k.mean = (((ci * 3) % 5 - 2) / xd).astype(F32)
    k.invstd = np.array([1.0, 0.5, 2.0] if mode == "fine" else [1.0, 0.5, 1.0], F32)[ci % 3]
    k._refs = {}
    return k


MUST_HOLD = ("y", "sum", "dy", "dx", "dW", "dbeta", "dgamma", "wino-V", "wino-U", "wino-y", "wino-dx", "wwg-Z", "wwg-dU", "wwg-dW")


def holds(b):
    return max(b[q] for q in MUST_HOLD) < EXACT


@functools.lru_cache(maxsize=None)
def mode_of(name):
    """the finest lattice whose every budget (sumsq apart: the GPU file bounds it where it does not hold) is below 2^24"""
    for mode in MODES:
        if holds(budget(_build(name, mode))):
            return mode
    raise AssertionError(f"{name}: no lattice keeps its reductions below 2^24")


@functools.lru_cache(maxsize=2)
def lattice_case(name):
    return _build(name, mode_of(name))


# -------------------------------------------------------------------------------------------------------- the reference
def in_view(k, view, dt=np.float64):
    """-> (activated input a, derivative mask of the producer's activation at its pre-activation)"""
    x = k.x.astype(dt)
    if view == "plain":
        return x, np.ones_like(x)
    z = x * k.scale.astype(dt) + k.shift.astype(dt)
    return O.act_fwd(z, view), O.act_mask(z, view)


def g_view(k, gview, dt=np.float64):
    g = k.g.astype(dt)
    if gview == "identity":
        return g
    y = k.yraw.astype(dt)
    s, t = k.gscale.astype(dt), k.gshift.astype(dt)
    return s * O.act_mask(s * y + t, gview) * g + (k.k1.astype(dt) * y + k.k0.astype(dt))


def _ref(k, key, make):
    if key not in k._refs:
        k._refs[key] = make()
    return k._refs[key]


def ref_fwd(k, view):
    """-> (y, per-channel sum of y, per-channel sum of y^2) in float64"""
    def make():
        y = O.conv2d_fwd(in_view(k, view)[0], k.w.astype(np.float64))
        return y, y.sum(axis=(0, 1, 2)), (y * y).sum(axis=(0, 1, 2))
    return _ref(k, ("fwd", view), make)


def _bwd(k, view, gview):
    return _ref(k, ("bwd", view, gview), lambda: O.conv2d_bwd(in_view(k, view)[0], k.w.astype(np.float64), g_view(k, gview))[:2])


def ref_dx(k, gview, accumulate=0):
    dx = _bwd(k, "plain", gview)[0]
    return dx + k.base.astype(np.float64) if accumulate else dx


def ref_dw(k, view, gview):
    return _bwd(k, view, gview)[1]


def ref_bn(k, view, gview):
    """ssdseg_conv3x3_bwd_data_bn -> (dx, dgamma, dbeta, k1, k0, (bound of k1, of k0))"""
    m = k.shape[0] * k.shape[1] * k.shape[2]
    dx = ref_dx(k, gview)
    mg = dx * in_view(k, view)[1]
    xhat = (k.x.astype(np.float64) - k.mean.astype(np.float64)) * k.invstd.astype(np.float64)
    dbeta, dgamma = mg.sum(axis=(0, 1, 2)), (mg * xhat).sum(axis=(0, 1, 2))
    sc, istd, mu = (v.astype(np.float64) for v in (k.scale, k.invstd, k.mean))
    k1 = -sc * dgamma * istd / m
    k0 = sc * (dgamma * istd * mu - dbeta) / m
    kbound = (U * np.abs(k1) + 2.0 ** -50 * np.abs(sc * dgamma * istd) / m,
              U * np.abs(k0) + 2.0 ** -50 * np.abs(sc) * (np.abs(dgamma * istd * mu) + np.abs(dbeta)) / m)
    return dx, dgamma, dbeta, k1, k0, kbound


def saved_copy(k, view, c_from, poison=np.nan):
    """the zero-bordered copy [n][h + 2][w + 2][cin] -> (as the test prepares it: channels [0, c_from) hold the activated input, the
    rest `poison`; as ssdseg_conv3x3_fwd_saved_from must leave it)"""
    n, h, w, cin, _ = k.shape
    a = in_view(k, view)[0].astype(F32)
    want = np.zeros((n, h + 2, w + 2, cin), F32)
    want[:, 1:-1, 1:-1] = a
    before = np.full_like(want, poison)
    before[..., :c_from] = want[..., :c_from]
    return before, want


# ------------------------------------------------------------------------------------------ Winograd in NumPy, any dtype
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
F2, F4 = (2, BT2, G2, AT2), (4, BT4, G4, AT4)


def _windows(x, m, dt):
    """(n, tiles_h, tiles_w, cin, m + 2, m + 2): the (m + 2)^2 input window of every m x m output tile, zero outside the image"""
    n, h, w, c = x.shape
    th, tw = cdiv(h, m), cdiv(w, m)
    xp = np.zeros((n, th * m + 2, tw * m + 2, c), dt)
    xp[:, 1:h + 1, 1:w + 1] = x
    return np.lib.stride_tricks.sliding_window_view(xp, (m + 2, m + 2), axis=(1, 2))[:, ::m, ::m]


def _untile(yt, h, w):
    n, th, tw, m, _, o = yt.shape
    return yt.transpose(0, 1, 3, 2, 4, 5).reshape(n, th * m, tw * m, o)[:, :h, :w]


def winograd(d, wgt, mats, dt=np.float64, absolute=False):
    """Y = A^T [ sum_c (G w_c G^T) . (B^T d_c B) ] A per tile, every stage held in dtype `dt` (float32: an emulation of the kernels'
    arithmetic up to the order of the sums); absolute: the same with |.| of every matrix and operand -- the sum of the absolute terms
    of every reduction on the way, the factor of the F(4x4) bound and of the F(2x2) budgets"""
    m, BT, G, AT = mats
    n, h, w, _ = d.shape
    if absolute:
        BT, G, AT, d, wgt = (np.abs(a) for a in (BT, G, AT, d, wgt))
    BT, G, AT = BT.astype(dt), G.astype(dt), AT.astype(dt)
    u = np.einsum("ik,klcn,jl->ijcn", G, wgt.astype(dt), G).astype(dt)
    v = np.einsum("ik,ntuckl,jl->ntuijc", BT, _windows(d.astype(dt), m, dt), BT).astype(dt)
    mm = np.einsum("ntuijc,ijco->ntuijo", v, u).astype(dt)
    return _untile(np.einsum("ik,ntuklo,jl->ntuijo", AT, mm, AT).astype(dt), h, w)


def flipped(wgt):
    """the filter of the input-gradient role: w[2 - i][2 - j][c][n] with the channel axes exchanged"""
    return wgt[::-1, ::-1].transpose(0, 1, 3, 2)


def wino_wgrad_abs(a, g):
    """-> (max |Z| = |A||dY||A^T|, sum_tiles |V| . |Z| (4, 4, cin, cout), |G^T| [.] |G| (3, 3, cin, cout)) of the Winograd weight gradient"""
    va = np.einsum("ik,ntuckl,jl->ntuijc", np.abs(BT2), _windows(np.abs(a), 2, np.float64), np.abs(BT2))
    n, h, w, o = g.shape
    th, tw = cdiv(h, 2), cdiv(w, 2)
    gp = np.zeros((n, th * 2, tw * 2, o))
    gp[:, :h, :w] = np.abs(g)
    gt = gp.reshape(n, th, 2, tw, 2, o).transpose(0, 1, 3, 2, 4, 5)
    za = np.einsum("ki,ntuklo,lj->ntuijo", np.abs(AT2), gt, np.abs(AT2))
    du = np.einsum("ntuijc,ntuijo->ijco", va, za)
    return za.max(), du, np.einsum("ki,klco,lj->ijco", np.abs(G2), du, np.abs(G2))


def budget(k):
    """sum of the absolute terms of every reduction a kernel forms, in units of the result's lattice; < 2^24 = every partial sum in any
    order, fused or not, is exact.  9 cin terms for y, 9 cout for dx, n h w for dW, for each statistics column and each fused sum
    (sumsq in units of the squared lattice); the statistics over the actual y of every input view; the backward over the worst view of
    each side (no clamp, every mask 1), accumulation base included.  The transformed domains of F(2x2, 3x3) (forward and input-gradient
    role) and of the Winograd weight gradient with the absolute matrices: V and Z on the data's lattice, U two halvings below the
    weights', sum_c U.V and its output transform on their product, sum_tiles V.Z on the data's square, its G^T . G two halvings below"""
    n, h, w, cin, cout = k.shape
    xd, wd = float(k.xd), float(k.wd)
    ua, uw = 1 / xd, 1 / wd
    x = np.abs(k.x.astype(np.float64))
    a = np.maximum(x, x * np.abs(k.scale) + np.abs(k.shift.astype(np.float64)))
    w64 = k.w.astype(np.float64)
    wa = np.abs(w64)
    yabs = O.conv2d_fwd(a, wa)
    out = {"y": yabs.max() / (ua * uw)}
    ssum = ssq = 0.0
    for view in ("plain", O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6):
        yv = ref_fwd(k, view)[0]
        ssum, ssq = max(ssum, np.abs(yv).sum(axis=(0, 1, 2)).max()), max(ssq, (yv * yv).sum(axis=(0, 1, 2)).max())
    out["sum"], out["sumsq"] = ssum / (ua * uw), ssq / (ua * uw) ** 2
    g = np.abs(k.g.astype(np.float64))
    udy = ua * ua
    dy = np.maximum(g, np.abs(k.gscale) * g + np.abs(k.k1 * k.yraw.astype(np.float64)) + np.abs(k.k0.astype(np.float64)))
    dxabs, dwabs, _ = O.conv2d_bwd(a, wa, dy)
    dxabs = dxabs + np.abs(k.base)
    xhat = (x + np.abs(k.mean)) * k.invstd
    out["dy"] = dy.max() / udy
    out["dx"] = dxabs.max() / (udy * uw)
    out["dW"] = dwabs.max() / (ua * udy)
    out["dbeta"] = dxabs.sum(axis=(0, 1, 2)).max() / (udy * uw)
    out["dgamma"] = (dxabs * xhat).sum(axis=(0, 1, 2)).max() / (udy * uw * ua / 2)
    # F(2x2, 3x3): the forward over a, the input gradient over the plain gradient (a BatchNorm gradient view goes to the implicit GEMM)
    out["wino-V"] = 4 * max(a.max() / ua, g.max() / ua)
    out["wino-U"] = np.einsum("ik,klcn,jl->ijcn", np.abs(G2), wa, np.abs(G2)).max() / (uw / 4)
    out["wino-y"] = winograd(a, w64, F2, absolute=True).max() / (ua * uw / 4)
    out["wino-dx"] = (winograd(g, flipped(w64), F2, absolute=True) + np.abs(k.base)).max() / (ua * uw / 4)
    zmax, du, dwg = wino_wgrad_abs(a, g)
    out["wwg-Z"], out["wwg-dU"], out["wwg-dW"] = zmax / ua, du.max() / (ua * ua), dwg.max() / (ua * ua / 4)
    return out


# ------------------------------------------------------------------------------------------------ the F(4x4, 3x3) bound
# roundings on the longest path of one 1-D pass, per ROW of the transform matrix, read from csrc/conv3_wino4.h (derivation in the
# docstring of tests/test_gpu_conv3_edges.py): G (conv3_wino4_weights_kernel), B^T (w4_bt_lo / w4_bt_hi), A^T (epilogue_round)
F4_G_ROUNDINGS = np.array([1, 3, 3, 3, 3, 0])
F4_G_CONSTANTS = np.array([0, 1, 1, 1, 1, 0])       # rows whose constants (1/6, 1/12, 1/24) are themselves rounded
F4_BT_ROUNDINGS = np.array([3, 2, 2, 2, 2, 2])
F4_AT_ROUNDINGS = np.array([3, 2, 2, 3])
F4_ROUNDINGS = 2 * 3 + 1 + 2 * 3 + 2 * 3            # the worst path through the three transforms and the view: 19
F4_SECOND_ORDER = 1 + 2.0 ** -10                    # products of two of the relative errors below (each <= 2^-18 of a first-order term)


def _pairs(r):
    return (r[:, None] + r[None, :]).astype(np.float64)


def f4_bound(d, d_abs, wgt, cred, viewed):
    """per output element, with U_c = G w_c G^T, V_c = B^T d_c B, M = sum_c U_c . V_c and |.|-matrices marked ':
        |A^T| [ sum_c ( eu . U'_c . |V_c|  +  ev . |U_c| . V'_c  +  gamma(cred) |U_c| . |V_c| ) ] |A|  +  ey . (|A^T| |M| |A|)
    eu, ev, ey: the roundings on the path to each POSITION of the 6 x 6 (4 x 4) grid times U = 2^-24.  d_abs: the absolute terms of
    the operand (|s x| + |t| under a view, whose one rounding ev counts; |d| for a plain tensor)"""
    m, BT, G, AT = F4
    n, h, w, _ = d.shape
    wgt = wgt.astype(np.float64)
    eu = U * (_pairs(F4_G_ROUNDINGS) + _pairs(F4_G_CONSTANTS))
    ev = U * (_pairs(F4_BT_ROUNDINGS) + (1 if viewed else 0))
    ey = U * _pairs(F4_AT_ROUNDINGS)
    u = np.einsum("ik,klcn,jl->ijcn", G, wgt, G)
    ua = np.einsum("ik,klcn,jl->ijcn", np.abs(G), np.abs(wgt), np.abs(G))
    v = np.einsum("ik,ntuckl,jl->ntuijc", BT, _windows(d.astype(np.float64), m, np.float64), BT)
    va = np.einsum("ik,ntuckl,jl->ntuijc", np.abs(BT), _windows(d_abs.astype(np.float64), m, np.float64), np.abs(BT))
    dm = np.einsum("ntuijc,ijco->ntuijo", np.abs(v), eu[:, :, None, None] * ua + gamma(cred) * np.abs(u)) + \
        np.einsum("ntuijc,ijco->ntuijo", va * ev[:, :, None], np.abs(u))
    mm = np.einsum("ntuijc,ijco->ntuijo", v, u)
    b = np.einsum("ik,ntuklo,jl->ntuijo", np.abs(AT), dm, np.abs(AT)) + ey[:, :, None] * np.einsum("ik,ntuklo,jl->ntuijo", np.abs(AT), np.abs(mm), np.abs(AT))
    return F4_SECOND_ORDER * _untile(b, h, w)


def f4_bound_issue(d_abs, wgt, cred):
    """the worst-path form: (gamma(cred + r) + 3 . 2U) |A^T| [ sum_c (|G||w_c||G^T|) . (|B^T||d_c||B|) ] |A|, r = F4_ROUNDINGS.  The
    emulation and the kernel stay below 0.01 of it, so the tests hold both to the per-position form above, which it dominates"""
    return (gamma(cred + F4_ROUNDINGS) + 6 * U) * winograd(d_abs, wgt, F4, absolute=True)


def view_abs(k, view):
    x = np.abs(k.x.astype(np.float64))
    return x if view == "plain" else x * np.abs(k.scale.astype(np.float64)) + np.abs(k.shift.astype(np.float64))


def f4_bound_fwd(k, view):
    return _ref(k, ("f4b", view), lambda: f4_bound(in_view(k, view)[0], view_abs(k, view), k.w, k.shape[3], view != "plain"))


def f4_bound_dx(k, accumulate=0):
    def make():
        g = k.g.astype(np.float64)
        b = f4_bound(g, np.abs(g), flipped(k.w), k.shape[4], False)
        return b + U * (np.abs(ref_dx(k, "identity")) + b + np.abs(k.base)) if accumulate else b
    return _ref(k, ("f4bdx", accumulate), make)


# ---- F(2x2, 3x3) off the lattice: additions and exact halvings only, so a rounding count on the worst path and the absolute matrices
F2_ROUNDINGS = 11        # 4 (U: two adds per pass, the halving is exact) + 1 (the view) + 2 (V: one add per pass) + 4 (A^T . A: two adds per pass)
F2_WGRAD_ROUNDINGS = 9   # 1 (the view) + 2 (V) + 2 (Z = A dY A^T: one add per pass) + 4 (G^T . G: two adds per pass, then the exact halving)


def f2_bound(d_abs, wgt, cred):
    return gamma(cred + F2_ROUNDINGS) * winograd(d_abs, wgt, F2, absolute=True)


def f2_wgrad_bound(k, view, slots):
    """gamma(tiles + slots + r) |G^T| [ sum_tiles |V| . |Z| ] |G|: a float32 chain over the tiles of a slab, the slab sum, the transforms"""
    n, h, w, _, _ = k.shape
    tiles = n * cdiv(h, 2) * cdiv(w, 2)
    return gamma(tiles + slots + F2_WGRAD_ROUNDINGS) * wino_wgrad_abs(view_abs(k, view), k.g.astype(np.float64))[2]


def f4_emulation(k, view):
    """float32 NumPy emulation of the three transforms and the channel sum of the forward"""
    return winograd(in_view(k, view, F32)[0], k.w, F4, dt=F32)


F4_CASES = [name for name, c in CASES.items() if any(s.startswith("wino4") for s in c["settings"])]

# ------------------------------------------------------------------------------------------------------ the normal family
NORMAL_CASES = ["px-9x33", "px-7x31", "col-fwd-164", "col-bwd-132", "wcol-fwd-68", "f4-5x5", "f4-two-blocks", "f4-cred48", "f4-plain", "gemm-straddle",
                "narrow-16x4", "direct-2x17", "wgt-68x68-w33", "wgt-uneven", "nine-36x132-17x32", "taps-36x36", "ww-tail-two", "ww-9x2x32"]
BAND = 1e-4


def _off_thresholds(v, s, t):
    z = v.astype(np.float64) * s + t
    near = (np.abs(z) < BAND) | (np.abs(z - 6) < BAND)
    return np.where(near, v + F32(0.05), v).astype(F32)


@functools.lru_cache(maxsize=2)
def normal_case(name):
    n, h, w, cin, cout = shape_of(name)
    rng = seeded(7, *[ord(ch) for ch in name])
    k = Case()
    k.name, k.shape, k.mode, k.ldx = name, (n, h, w, cin, cout), "normal", ldx_of(name)
    k.scale = (rng.uniform(0.5, 1.5, cin) * rng.choice([-1.0, 1.0], cin, p=[0.25, 0.75])).astype(F32)
    k.shift = rng.uniform(-1, 3, cin).astype(F32)
    k.gscale = rng.uniform(0.5, 1.5, cout).astype(F32)
    k.gshift = rng.uniform(-1, 3, cout).astype(F32)
    k.x = _off_thresholds(rng.normal(0, 2, (n, h, w, cin)).astype(F32), k.scale, k.shift)
    k.yraw = _off_thresholds(rng.normal(0, 2, (n, h, w, cout)).astype(F32), k.gscale, k.gshift)
    k.w = (rng.normal(0, 1, (3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(F32)
    k.g = rng.normal(0, 2, (n, h, w, cout)).astype(F32)
    k.base = rng.normal(0, 2, (n, h, w, cin)).astype(F32)
    k.k1 = rng.normal(0, 0.1, cout).astype(F32)
    k.k0 = rng.normal(0, 0.1, cout).astype(F32)
    k.mean = k.x.mean(axis=(0, 1, 2), dtype=np.float64).astype(F32)
    k.invstd = (1.0 / np.sqrt(k.x.var(axis=(0, 1, 2), dtype=np.float64) + 1e-3)).astype(F32)
    k._refs = {}
    return k


def normal_bounds(k, view, gview, accumulate=0, dx_b=None):
    """any-order per-element and per-channel bounds of one form of a normal case (derivations: tests/test_gpu_conv3_edges.py); dx_b: the
    bound of dx where a Winograd form computed it (the fused sums are built on it)"""
    n, h, w, cin, cout = k.shape
    m = n * h * w
    za = view_abs(k, view)
    _, mask = in_view(k, view)
    wa = np.abs(k.w.astype(np.float64))
    y = ref_fwd(k, view)[0]
    y_b = (gamma(9 * cin + 1) + U) * O.conv2d_fwd(za, wa)
    sum_b = gamma(m + 1) * np.abs(y).sum(axis=(0, 1, 2)) + y_b.sum(axis=(0, 1, 2))
    g, yr = k.g.astype(np.float64), k.yraw.astype(np.float64)
    dabs = np.abs(g) if gview == "identity" else np.abs(k.gscale * g) + np.abs(k.k1 * yr) + np.abs(k.k0.astype(np.float64))
    dxa, dwa, _ = O.conv2d_bwd(za, wa, dabs)
    dx = ref_dx(k, gview, accumulate)
    plain_dx = dx_b is None
    if plain_dx:
        dx_b = (gamma(9 * cout + 1) + 2 * U) * dxa
    if accumulate and plain_dx:
        dx_b = dx_b + U * (np.abs(ref_dx(k, gview)) + np.abs(k.base.astype(np.float64)) + dx_b)
    dw = ref_dw(k, view, gview)
    dw_b = (gamma(m + 2) + 3 * U) * dwa + gamma(2) * np.abs(dw)
    x = k.x.astype(np.float64)
    xhat = np.abs((x - k.mean) * k.invstd)
    mdx = np.abs(dx * mask)
    dbeta_b = gamma(m + 1) * mdx.sum(axis=(0, 1, 2)) + (dx_b * mask).sum(axis=(0, 1, 2)) + U * np.abs((dx * mask).sum(axis=(0, 1, 2)))
    dgamma_b = (gamma(m + 2) + 2 * U) * (mdx * xhat).sum(axis=(0, 1, 2)) + (dx_b * mask * xhat).sum(axis=(0, 1, 2)) + \
        U * np.abs((dx * mask * (x - k.mean) * k.invstd).sum(axis=(0, 1, 2)))
    return dict(y=y_b, sum=sum_b, dx=dx_b, dW=dw_b, dbeta=dbeta_b, dgamma=dgamma_b)


def sumsq_bound(y, y_b):
    """sum of y^2 over m = n h w pixels from y within y_b: gamma(m + 2) sum y^2 + sum (2 |y| b + b^2)"""
    m = y.shape[0] * y.shape[1] * y.shape[2]
    return gamma(m + 2) * (y * y).sum(axis=(0, 1, 2)) + (2 * np.abs(y) * y_b + y_b * y_b).sum(axis=(0, 1, 2))


# what the suite must reach: every 3x3 kernel symbol tests/test_gpu_conv3_dispatch.py lists as reachable at small shapes
def coverage_gaps(seen):
    want = [r"^conv3_tile_kernel<%d> \[%s\]$" % (wn, role) for wn in range(1, 6) for role in ("fwd", "bwd_data")]
    want += [r"^conv3_wino_kernel<true> \[fwd\]$", r"^conv3_wino_kernel<false> \[fwd\]$", r"^conv3_wino_kernel<false> \[bwd_data\]$",
             r"^conv3_wino4_kernel<true> \[fwd\]$", r"^conv3_wino4_kernel<false> \[fwd\]$", r"^conv3_wino4_kernel<false> \[bwd_data\]$",
             r"^conv3_wino_weights_kernel$", r"^conv3_wino4_weights_kernel$", r"^conv3_wino_wgrad_kernel$", r"^conv3_wino_wgrad_finalize_kernel$",
             r"^conv3_wgrad_tile_kernel$", r"conv3_wgrad12_kernel", r"conv3_wgrad9_kernel<1>", r"conv3_wgrad9_kernel<4>", r"^conv3n_tapsum_kernel$",
             r"^conv3n_shift_kernel$", r"^conv3n_pack_w_kernel$", r"^conv3n_bwd_bn_direct_kernel$", r"^conv3n_dymat_kernel$", r"^conv3_pad_view_kernel$",
             r"^conv3_transpose_w_kernel$", r"^colsum_kernel$", r"^gemm_rowA_kernel<\d, 0, 1, ", r"^gemm_rowA_kernel<\d, 1, 1, ",
             r"^gemm_wgrad_kernel<.*\[conv3x3 tap\]$"]
    return [p for p in want if not reaches(seen, p)]
