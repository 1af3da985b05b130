"""Named edge cases, the float64 reference, bounds and a mirror of the host rules for the pointwise (1x1) conv GEMMs: plain NumPy.

The entry points are ssdseg_pwconv_parts, ssdseg_pwconv_fwd / _fwd_wt, ssdseg_pwconv_bwd_data, ssdseg_pwconv_bwd_weight,
ssdseg_pwconv_bwd and ssdseg_pwconv_bwd_bn (csrc/gemm.hip with csrc/gemm_wres.h and csrc/pw_tile.h; csrc/pw_wgrad.hip with
csrc/pw_wgrad.h).  tests/test_cpu_pw_cases.py vets the reference, the cases and the mirror on the CPU; tests/test_gpu_pw_edges.py
runs the kernels on the same cases.  Every builder seeds its own generator from its arguments, so the same call gives the same
arrays in both files.  Shapes are (m, k, n): rows, input channels, output channels.

The lattice family.  Every input is a small multiple of a power of two, so that every product and every sum of the GEMMs, of both
views and of all reductions is a float32 number whatever the order and whether or not a multiply-add is fused (the MFMA has exact
fp32 products): the float64 reference IS the float32 result and the bound is 0.  `fine`: x, g, yraw, the shifts, k1, k0 and mean are
multiples of 1/4, weights of 1/8; `coarse`: integers and weights that are multiples of 1/2; `thin`: coarse with one x / g value in
four non-zero; `sparse` (every case of 65,000 rows and more): integers, one value in eight non-zero, no shifts.  A smaller case takes the
finest mode whose `budget` stays below 2^24 everywhere.  Scales and invstd are signed powers of two.  `budget` gives, in units of each result's
lattice, the sum of the absolute terms of every reduction; below 2^24 no partial sum in any order leaves the integers float32 holds
exactly.  The (scale, shift) pairs put many pre-activations exactly on 0 and exactly on 6 in both views: nothing is nudged.

The normal family.  N(0, 2) data off the lattice, pre-activations kept out of a 1e-4 band around 0 and 6, derived any-order bounds
(U = 2^-24, gamma(L) = L U / (1 - L U)); the derivations stand in the docstring of tests/test_gpu_pw_edges.py.

The mirror.  pick_wn / rowA_grid_y_wn (csrc/gemm_internal.h, csrc/gemm.hip), pw_tile_takes / pwt_short_ncols / the ncols and wave
choice of pw_tile_launch, the tile-shape choice and split count of pw_wgrad_try / pw_wgrad_launch and of the general weight
gradient: what decides which kernel runs and how many partial rows it writes -- not the accumulation order.
"""
import functools

import numpy as np

from oracle import np_ops as O

F32 = np.float32
U = 2.0 ** -24
EXACT = 2 ** 24
ACTS = (O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6, O.ACT_ZERO)
ACT_NAMES = {O.ACT_NONE: "none", O.ACT_RELU: "relu", O.ACT_RELU6: "relu6", O.ACT_ZERO: "zero"}
ONCE_ENV = ("SSDSEG_WRES_LDS_KB",)           # read once per process: must be unset
# every switch the pointwise host code reads per call (the GPU file clears them all before it sets a setting)
PW_VARS = ("SSDSEG_NO_WRES", "SSDSEG_WRES_FORCE", "SSDSEG_PW_FUSED", "SSDSEG_PW_TILE", "SSDSEG_PW_WGRAD", "SSDSEG_OCC_ROWS",
           "SSDSEG_PWT_SMALL", "SSDSEG_PW_TILE_BIG_ROWS", "SSDSEG_PWT_GRID", "SSDSEG_NO_F4_EPILOGUE", "SSDSEG_NO_BN_EPILOGUE",
           "SSDSEG_ROWA_PARTS", "SSDSEG_PWT_PARTS", "SSDSEG_ROWA_BWD_WN", "SSDSEG_ROWA_WN_MAX", "SSDSEG_WGRAD_SLAB_FRAC",
           "SSDSEG_WGRAD_BPC", "SSDSEG_WGRAD_BPC_LONG")
_ROWA = {"SSDSEG_NO_WRES": "1", "SSDSEG_PW_TILE": "0", "SSDSEG_PW_WGRAD": "0"}
SETTINGS = {
    "default": {},
    "rowA": dict(_ROWA),
    "rowA-occ": dict(_ROWA, SSDSEG_OCC_ROWS="0"),
    "rowA-fused": dict(_ROWA, SSDSEG_PW_FUSED="1"),
    "rowA-fused-occ": dict(_ROWA, SSDSEG_OCC_ROWS="0", SSDSEG_PW_FUSED="1"),
    "resident": {"SSDSEG_WRES_FORCE": "1", "SSDSEG_PW_FUSED": "1", "SSDSEG_PW_TILE": "0"},
    "tile": {"SSDSEG_PW_TILE": "1"},
    "tile-32": {"SSDSEG_PW_TILE": "1", "SSDSEG_PWT_SMALL": "32"},
    "tile-big": {"SSDSEG_PW_TILE": "1", "SSDSEG_PWT_SMALL": "0", "SSDSEG_PW_TILE_BIG_ROWS": "0"},
    "tile-big-nogrid": {"SSDSEG_PW_TILE": "1", "SSDSEG_PWT_SMALL": "0", "SSDSEG_PW_TILE_BIG_ROWS": "0", "SSDSEG_PWT_GRID": "0"},
    "scalar": {"SSDSEG_NO_F4_EPILOGUE": "1", "SSDSEG_NO_BN_EPILOGUE": "1", "SSDSEG_PW_TILE": "0"},
    "parts64": {"SSDSEG_ROWA_PARTS": "64", "SSDSEG_PWT_PARTS": "64"},
}


def gamma(length):
    return length * U / (1.0 - length * U)


def seeded(*key):
    return np.random.default_rng([1993, 1101] + [int(k) for k in key])


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================= mirror of the host rules
BM, BK, AS = 128, 32, 36
ROWA_OCC_ROWS = 150000
NUM_CUS = 256                  # the MI355X: the fused kernels and the weight gradient size their grids by it
PWT_SHORT_ROWS = 65536


def _is(env, name, ch):
    return env.get(name, "")[:1] == ch


def _int(env, name, fallback):
    return int(env[name]) if name in env else fallback


def pick_wn(n, row_blocks):
    best, best_pad, best_blocks, best_full = 1, -1, -1, False
    for wn in range(1, 6):
        tiles = cdiv(n, 32 * wn)
        pad, blocks = tiles * 32 * wn, tiles * row_blocks
        full = blocks >= 512
        if best_pad < 0:
            take = True
        elif full != best_full:
            take = full
        elif full:
            take = pad <= best_pad
        else:
            take = blocks > best_blocks or (blocks == best_blocks and pad <= best_pad)
        if take:
            best, best_pad, best_blocks, best_full = wn, pad, blocks, full
    return best


def occ_rows(env):
    return _int(env, "SSDSEG_OCC_ROWS", ROWA_OCC_ROWS)


def rowA_wn(rows, cols, env):
    wn = pick_wn(cols, cdiv(rows, BM))
    cap = _int(env, "SSDSEG_ROWA_WN_MAX", 0)
    return cap if cap >= 1 and wn > cap else wn


def rowA_wn_bwd(rows, cols, red, env):
    wn = rowA_wn(rows, cols, env)
    cap = _int(env, "SSDSEG_ROWA_BWD_WN", 3)
    return cap if (cap >= 1 and rows >= occ_rows(env) and red <= 48 and wn > cap) else wn


def rowA_grid_y_wn(rows, cols, wn, env):
    ntiles, mtiles = cdiv(cols, 32 * wn), cdiv(rows, BM)
    parts = _int(env, "SSDSEG_ROWA_PARTS", 0)
    cap = parts if parts >= 64 else (1024 if wn == 1 else 512)
    if mtiles * ntiles <= 2 * cap:
        return mtiles
    gy = max(cap // ntiles, 1)
    if mtiles <= gy:
        return mtiles
    return cdiv(mtiles, cdiv(mtiles, gy))


def rowA_grid_y(rows, cols, env):
    """== ssdseg_pwconv_parts: rows of the statistics table"""
    return rowA_grid_y_wn(rows, cols, rowA_wn(rows, cols, env), env)


def wres_lds_bytes(r, wn):
    rp = cdiv(r, BK) * BK
    b = (rp * (32 * wn + 1) + 4 * rp + 4 * 32 * AS) * 4
    return b if b <= 64 * 1024 else 0


def wres_mode(env):
    return 0 if _is(env, "SSDSEG_NO_WRES", "1") else (2 if _is(env, "SSDSEG_WRES_FORCE", "1") else 1)


def pw_tile_mode(env):
    return 2 if "SSDSEG_PW_TILE" not in env else (0 if _is(env, "SSDSEG_PW_TILE", "0") else 1)


def pw_tile_default(mode, rows, cred, nout, fused_bn, accumulate, env):
    pinned = _is(env, "SSDSEG_PWT_SMALL", "0")
    if mode == 0:
        return nout >= 256 or (rows >= 500000 and cred >= 256) or (rows < 65536 and not pinned)
    if not fused_bn and not accumulate and rows <= 16384 and not pinned:
        return True
    return not fused_bn and not accumulate and cred <= 384 and (nout >= 256 or cred >= 256)


def pw_tile_takes(rows, lda, cred, nout):
    return cred % 8 == 0 and cred >= 64 and nout % 4 == 0 and rows * lda * 4 < (1 << 31) and nout * cred * 4 < (1 << 31)


def pw_tile_wanted(mode, rows, lda, cred, nout, fused_bn, adds, env):
    sw = pw_tile_mode(env)
    return sw != 0 and pw_tile_takes(rows, lda, cred, nout) and (sw == 1 or pw_tile_default(mode, rows, cred, nout, fused_bn, adds, env))


def pwt_short_ncols(mode, rows, cred, nout, env):
    if "SSDSEG_PWT_SMALL" in env:
        nc = int(env["SSDSEG_PWT_SMALL"])
        return nc if nc >= 32 else 0
    t64 = cdiv(nout, 64)
    pad64 = cdiv((cdiv(nout, t64) + 3) // 4 * 4, 32) * 32 * t64 * 4 > nout * 5
    if mode == 0:
        if rows <= 16384:
            return 0 if nout >= 512 else 32
        if cred <= 64:
            return 128
        return 32 if (nout <= 64 or pad64) else 64
    if rows <= 16384:
        return 32
    return 64 if nout <= 64 else (32 if pad64 else 64)


def pwt_part_rows(rows, block_rows, gx, env):
    mtiles = cdiv(rows, block_rows)
    parts = _int(env, "SSDSEG_PWT_PARTS", 0)
    cap = (parts if parts >= 64 else 1024 * gx) // gx
    return max(min(mtiles, cap), 1)


def pw_tile_plan(mode, rows, cred, nout, env, nparts_y=0):
    """pw_tile_launch -> dict(symbol, waves, wn, wnw, ncols, gx, gy, block_rows)"""
    ntiles = 1 if nout <= 160 else cdiv(nout, 256)
    if rows < PWT_SHORT_ROWS:
        nc = pwt_short_ncols(mode, rows, cred, nout, env)
        if nc > 0:
            ntiles = cdiv(nout, nc)
    ncols = (cdiv(nout, ntiles) + 3) // 4 * 4
    wn = cdiv(ncols, 32)
    big = rows >= _int(env, "SSDSEG_PW_TILE_BIG_ROWS", 65536)
    if (not big or mode == 1) and wn > 5:
        ncols = (cdiv(nout, cdiv(nout, 160)) + 3) // 4 * 4
        wn = cdiv(ncols, 32)
    grid42 = mode == 1 and big and 160 < nout <= 256 and not _is(env, "SSDSEG_PWT_GRID", "0")
    if grid42:
        ncols = (nout + 3) // 4 * 4
        wn = cdiv(ncols, 64)
    gx = cdiv(nout, ncols)
    block_rows = 256 if (big and not grid42) else 128
    gy = nparts_y if nparts_y > 0 else pwt_part_rows(rows, block_rows, gx, env)
    if grid42:
        waves, tw, wnw = 8, (3 if wn <= 3 else 4), 2
    elif big and (wn <= 5 or mode == 0):
        waves, wnw = 8, 1
        tw = 2 if wn <= 2 else (4 if wn <= 4 else (5 if wn == 5 else (6 if wn == 6 else 8)))
    else:
        waves, tw, wnw = 4, min(max(wn, 1), 5), 1
    symbol = f"pw_tile_kernel<{waves}, {tw}, {mode}" + (f", {wnw}>" if wnw != 1 else ">")
    return dict(symbol=symbol, waves=waves, wn=tw, wnw=wnw, ncols=ncols, gx=gx, gy=gy, block_rows=block_rows, grid42=grid42,
                last_cols=nout - (gx - 1) * ncols, row_tiles=cdiv(rows, block_rows), last_rows=rows - (cdiv(rows, block_rows) - 1) * block_rows)


def rowa_plan(mode, rows, red, cols, lda, env, coef=False, adds=False, aligned=True, wt_copy=False, stats=False):
    """launch_rowA<MODE, 0> -> ({symbol: launches}, geometry).  mode 0: forward (cols = n, red = k); mode 1: input gradient
    (cols = k, red = n).  `coef`: the streamed operand carries view coefficients; `aligned`: the output (and residual) pointer and
    pitch allow the float4 epilogue"""
    wn = rowA_wn_bwd(rows, cols, red, env) if mode == 1 else rowA_wn(rows, cols, env)
    nparts = rowA_grid_y(rows, cols, env)
    if not (mode == 0 and adds) and pw_tile_wanted(mode, rows, lda, red, cols, False, adds, env):
        t = pw_tile_plan(mode, rows, red, cols, env, nparts if stats else 0)     # (with statistics: one block per table row)
        launches = {t["symbol"]: 1}
        if mode == 0 and not wt_copy:
            launches["conv3_transpose_w_kernel"] = 1
        return launches, dict(t, family="tile")
    grid_y = rowA_grid_y_wn(rows, cols, wn, env) if mode == 1 else nparts
    if mode == 1 and coef and red >= 256:
        wide, mtiles = cdiv(cols, 32), cdiv(rows, BM)
        if wide > wn and wide <= 3 and mtiles >= 256 and rows < ROWA_OCC_ROWS:
            wn, grid_y = wide, min(mtiles, 2048)
    geom = dict(wn=wn, gx=cdiv(cols, 32 * wn), gy=grid_y, row_tiles=cdiv(rows, BM), last_rows=rows - (cdiv(rows, BM) - 1) * BM,
                last_cols=cols - (cdiv(cols, 32 * wn) - 1) * 32 * wn, nparts=nparts)
    wm = wres_mode(env)
    if wres_lds_bytes(red, wn) > 0 and (wm == 2 or (wm == 1 and rows >= 500000 and not (mode == 1 and wn >= 4))):
        return {f"gemm_wres_kernel<{wn}, {mode}, 0>": 1}, dict(geom, family="resident")
    occ = int(rows >= occ_rows(env))
    ep = int(wn >= 2 and not _is(env, "SSDSEG_NO_F4_EPILOGUE", "1") and cols % 4 == 0 and aligned)
    return {f"gemm_rowA_kernel<{wn}, {mode}, 0, 0, {ep}, {occ}>": 1}, dict(geom, family="rowA", ep=ep, occ=occ)


PWW_SHAPES = [(256, 128, (2, 2, 4, 2)), (128, 256, (2, 2, 2, 4)), (128, 128, (2, 2, 2, 2)), (256, 64, (2, 2, 4, 1)), (64, 128, (2, 2, 1, 2)),
              (128, 64, (2, 2, 2, 1)), (256, 32, (4, 1, 2, 1)), (64, 64, (2, 2, 1, 1)), (32, 128, (1, 4, 1, 1)), (128, 32, (4, 1, 1, 1)),
              (32, 64, (1, 2, 1, 1)), (64, 32, (2, 1, 1, 1)), (32, 32, (1, 1, 1, 1))]


def pww_ms(kt, nt):
    return 16 if kt + nt > 256 else (32 if kt + nt > 128 else 64)


def _slab_fraction(env):
    f = float(env.get("SSDSEG_WGRAD_SLAB_FRAC", 0.5))
    return f if f > 0 else 0.5


def wgrad_plan(m, k, n, ldx, ldy, env):
    """wgrad_run -> ({symbol: launches}, geometry): the row-naming kernel (pw_wgrad_try / pw_wgrad_launch) or the general one"""
    frac = _slab_fraction(env)
    row_naming = not _is(env, "SSDSEG_PW_WGRAD", "0") and k % 4 == 0 and n % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and \
        (m + 64) * ldx * 4 < (1 << 31) and (m + 64) * ldy * 4 < (1 << 31)
    if row_naming:
        best, best_t = None, 0.0
        for kt, nt, inst in PWW_SHAPES:
            tk, tn = float(cdiv(k, kt)), float(cdiv(n, nt))
            t_mfma = 2.0 * m * (tk * kt) * (tn * nt) / 110e12
            t_hbm = 4.0 * m * (float(k) * tn + float(n) * tk) / 4.5e12
            t = max(t_mfma, t_hbm)
            if best is None or t < best_t * 0.999:
                best, best_t = (kt, nt, inst), t
        kt, nt, inst = best
        ms = pww_ms(kt, nt)
        ktiles, ntiles = cdiv(k, kt), cdiv(n, nt)
        steps = cdiv(m, ms)
        splits = cdiv(2 * NUM_CUS, ktiles * ntiles)
        splits = min(splits, cdiv(steps, 4), int(float(m) * (k + n) * frac / (float(k) * n)))
        splits = min(max(splits, 1), 65535)
        sps = cdiv(steps, splits)
        splits = cdiv(steps, sps)
        symbol = "pw_wgrad_kernel<%d, %d, %d, %d>" % inst
        step_rows = ms
    else:
        wi = 1 if k <= 32 else (2 if k <= 64 else 4)
        wr = 4 // wi
        brt = (16 if wr == 4 else 32) * wr
        itiles = cdiv(k, 32 * wi)
        steps = cdiv(m, brt)
        max_splits = cdiv(steps, 4)
        cap = int(float(m) * (k + n) * frac / (float(k) * n))
        if max_splits > cap:
            max_splits = max(cap, 1)
        wn = pick_wn(n, itiles * max_splits)
        if wi == 1 and wn > 3:
            wn = 3
        jtiles = cdiv(n, 32 * wn)
        bpc = _int(env, "SSDSEG_WGRAD_BPC_LONG", 4) if m >= ROWA_OCC_ROWS else _int(env, "SSDSEG_WGRAD_BPC", 2)
        want = cdiv(bpc * NUM_CUS, itiles * jtiles)
        splits = min(max(1, min(want, max_splits)), 65535)
        sps = cdiv(steps, splits)
        splits = cdiv(steps, sps)
        symbol = f"gemm_wgrad_kernel<{wi}, {wr}, {wn}>"
        kt, nt, ktiles, ntiles, step_rows = 32 * wi, 32 * wn, itiles, jtiles, brt
    rps = sps * step_rows
    launches = {symbol: 1}
    if splits > 1:
        launches["colsum_kernel"] = 1
    return launches, dict(symbol=symbol, row_naming=row_naming, kt=kt, nt=nt, ktiles=ktiles, ntiles=ntiles, ms=step_rows, steps=steps,
                          splits=splits, rows_per_split=rps, last_split_rows=m - (splits - 1) * rps)


def fused_taken(m, k, n, env):
    force, never = _is(env, "SSDSEG_PW_FUSED", "1"), _is(env, "SSDSEG_PW_FUSED", "0")
    return not never and k <= 32 and n <= 192 and (force or (n > 32 and m >= 500000))


def merge(*launches):
    out = {}
    for l in launches:
        for s, c in l.items():
            out[s] = out.get(s, 0) + c
    return out


def plan_fwd(m, k, n, ldx, env, wt_copy=False, aligned=True, stats=False):
    return rowa_plan(0, m, k, n, ldx, env, aligned=aligned, wt_copy=wt_copy, stats=stats)


def plan_bwd_data(m, k, n, ldy, env, coef, adds, aligned=True):
    return rowa_plan(1, m, n, k, ldy, env, coef=coef, adds=adds, aligned=aligned)


def plan_bwd(m, k, n, ldx, ldy, env, coef, adds, aligned=True):
    """ssdseg_pwconv_bwd -> ({symbol: launches}, geometry of the fused launch or None)"""
    if not fused_taken(m, k, n, env):
        return merge(wgrad_plan(m, k, n, ldx, ldy, env)[0], plan_bwd_data(m, k, n, ldy, env, coef, adds, aligned)[0]), None
    nt, mtiles = cdiv(n, 32), cdiv(m, BM)
    gy = min(2 * NUM_CUS, mtiles)
    if wres_mode(env) != 0 and wres_lds_bytes(n, 1) > 0:
        symbol, wave_tiles, walkers = f"gemm_wres_kernel<1, 1, {nt}>", cdiv(m, 32), 4 * gy
    else:
        symbol, wave_tiles, walkers = f"gemm_rowA_kernel<1, 1, 0, {nt}, 0, {int(m >= occ_rows(env))}>", mtiles, gy
    launches = {symbol: 1}
    if gy > 1:
        launches["colsum_kernel"] = 1
    return launches, dict(symbol=symbol, nt=nt, gy=gy, tiles=wave_tiles, walkers=walkers, trips=cdiv(wave_tiles, walkers),
                          second_trip=max(wave_tiles - walkers, 0))


def plan_bwd_bn(m, k, n, ldx, ldy, env, coef, aligned=True):
    """ssdseg_pwconv_bwd_bn -> ({symbol: launches}, geometry): the weight gradient, then the input gradient with the sums in its
    epilogue, or (unaligned dx / SSDSEG_NO_BN_EPILOGUE) the plain input gradient and the reduction of ssdseg_bn_bwd_reduce"""
    w = wgrad_plan(m, k, n, ldx, ldy, env)[0]
    if not aligned or _is(env, "SSDSEG_NO_BN_EPILOGUE", "1"):
        d, geom = plan_bwd_data(m, k, n, ldy, env, coef, False, aligned)
        return merge(w, d, {"bn_bwd_partial_kernel": 1, "bn_bwd_finalize_kernel": 1}), dict(geom, fused=False)
    if pw_tile_wanted(1, m, ldy, n, k, True, False, env):
        nparts = pwt_part_rows(m, 256 if m >= 65536 else 128, 1, env)
        t = pw_tile_plan(1, m, n, k, env, nparts)
        return merge(w, {t["symbol"]: 1, "bn_bwd_finalize_kernel": 1}), dict(t, family="tile", fused=True)
    wn = rowA_wn_bwd(m, k, n, env)
    nparts = rowA_grid_y_wn(m, k, wn, env)
    symbol = f"gemm_rowA_kernel<{wn}, 1, 0, 0, 2, {int(m >= occ_rows(env))}>"
    return merge(w, {symbol: 1, "bn_bwd_finalize_kernel": 1}), dict(family="rowA", wn=wn, gy=nparts, fused=True, symbol=symbol)


# ============================================================================================================ the cases
# name: dict(shape, settings, entries, forms "all" | "large", ld (pitches) or None, kernel (what the case is there for))
CASES = {}
ALL_ENTRIES = ("fwd", "bwd_data", "bwd_weight", "bwd", "bwd_bn")


def _case(name, shape, settings, entries=ALL_ENTRIES, kernel="", ld=None):
    assert name not in CASES, name
    m = shape[0]
    CASES[name] = dict(shape=tuple(shape), settings=tuple(settings), entries=tuple(entries), forms="large" if m >= 65000 else "all",
                       ld=ld, kernel=kernel)


# rows: one row, the 32-row wave tile, the 128-row block tile, the 256-row eight-wave tile, a last tile holding one row
for _m in (1, 31, 32, 33, 127, 128, 129, 255, 256, 257):
    _case(f"rows{_m}-16x96", (_m, 16, 96), ("default", "rowA", "resident"), kernel="gemm_rowA_kernel<1, ")
    _case(f"rows{_m}-64x64", (_m, 64, 64), ("default", "rowA", "resident", "tile", "tile-big"), kernel="pw_tile_kernel<8, 2, ")
# reduction length of the rowA / resident kernels: below, at and above one and two 32-deep steps
for _r in (4, 28, 32, 36, 60, 64, 68):
    _case(f"red-k{_r}", (130, _r, 36), ("rowA", "resident"), ("fwd", "bwd_weight"), kernel="gemm_rowA_kernel<1, 0, ")
    _case(f"red-n{_r}", (130, 36, _r), ("rowA", "resident"), ("bwd_data", "bwd", "bwd_bn"), kernel="gemm_rowA_kernel<1, 1, ")
# reduction length of the tile GEMM: two steps, two + 8, three, three + 8; 56 and 60 are refused (below 64 / not a multiple of 8)
for _r in (56, 60, 64, 72, 96, 104):
    _case(f"tile-k{_r}", (130, _r, 64), ("tile",), ("fwd",), kernel="pw_tile_kernel<4, 1, 0>" if _r >= 64 else "gemm_rowA_kernel<1, 0, ")
    _case(f"tile-n{_r}", (130, 64, _r), ("tile",), ("bwd_data", "bwd_bn"), kernel="pw_tile_kernel<4, 1, 1>" if _r >= 64 else "gemm_rowA_kernel<1, 1, ")
# the last reduction that fits 64 KiB of LDS at one column tile, and the first that does not
_case("fit-288", (130, 288, 32), ("resident",), ("fwd",), kernel="gemm_wres_kernel<1, 0, 0>")
_case("fit-320", (130, 320, 32), ("resident",), ("fwd",), kernel="gemm_rowA_kernel<1, 0, ")
# columns: ragged last column tile of the rowA / resident kernels
for _n in (4, 28, 32, 36, 100, 160, 164):
    _case(f"cols{_n}", (130, 16, _n), ("default", "rowA", "resident"), ("fwd", "bwd_weight"), kernel="gemm_rowA_kernel<1, 0, ")
    _case(f"cols-k{_n}", (130, _n, 16), ("default", "rowA", "resident"), ("bwd_data", "bwd_bn"), kernel="gemm_rowA_kernel<1, 1, ")
# columns of the tile GEMM: the 32- / 64- / 128-column short-M rule, eight-wave WN = 2, 4, 5, 6, 8 and two tiles of 132
for _n in (64, 128, 160, 192, 256, 260):
    _case(f"tcols{_n}", (130, 64, _n), ("tile", "tile-32", "tile-big"), ("fwd",), kernel="pw_tile_kernel<8, ")
# the 4 x 2 wave grid: three- and four-tile waves, 36 and 8 ragged columns in the second wave group, and the same without the grid
for _m in (129, 257):
    for _k in (164, 200, 256):
        _case(f"grid42-{_m}x{_k}", (_m, _k, 64), ("tile-big", "tile-big-nogrid"), ("bwd_data", "bwd_bn"), kernel="pw_tile_kernel<8, ")
# wide rowA tiles: 514 row tiles (the last with one row) make every width "full": WN = 2..5, OCC 0 and 1, every epilogue
for _n in (60, 64, 92, 96, 100, 128, 160):
    _case(f"wide-n{_n}", (65665, 16, _n), ("rowA", "rowA-occ", "resident", "scalar"), ("fwd",), kernel="gemm_rowA_kernel<")
    _case(f"wide-k{_n}", (65665, _n, 16), ("rowA", "rowA-occ", "resident", "scalar"), ("bwd_data", "bwd_bn"), kernel="gemm_rowA_kernel<")
# the same beyond the cap (reduction 64 > 48): the occupancy-limited float4 and BatchNorm epilogues at WN = 4 and 5
for _k in (128, 160):
    _case(f"wide-k{_k}-n64", (65665, _k, 64), ("rowA-occ",), ("bwd_data", "bwd_bn"), kernel=f"gemm_rowA_kernel<{_k // 32}, 1, 0, 0, 2, 1>")
# grid-stride: 130 row tiles on 64 slots, second and third trips, the last on a one-row tile
_case("stride-16x32", (16513, 16, 32), ("parts64",), ("fwd", "bwd_data", "bwd_bn"), kernel="gemm_rowA_kernel<1, ")
_case("stride-64x64", (16513, 64, 64), ("parts64",), ("fwd", "bwd_data", "bwd_bn"), kernel="pw_tile_kernel<4, ")
# fused dx + dW: NT = 1..6 with ragged k and n; the two refusals run the separate kernels
FUSED_KN = ((4, 32), (16, 36), (16, 64), (16, 96), (28, 100), (32, 128), (24, 160), (32, 192))
for _m in (1, 33, 129, 640):
    for _k, _n in FUSED_KN:
        _case(f"fused-{_m}x{_k}x{_n}", (_m, _k, _n), ("resident", "rowA-fused", "rowA-fused-occ"), ("bwd",), kernel="gemm_wres_kernel<1, 1, ")
    for _k, _n in ((36, 96), (16, 196)):
        _case(f"unfused-{_m}x{_k}x{_n}", (_m, _k, _n), ("resident", "rowA-fused"), ("bwd",), kernel="gemm_wgrad_kernel<")
# fused, several tiles per wave: 2,053 wave tiles on 2,048 waves (NT = 2, 3, 4 in the two-steps-in-flight form); block-level
# grid-stride of the rowA form (514 row tiles on 512 blocks)
for _k, _n in ((8, 64), (16, 96), (32, 128)):
    _case(f"fused-walk-{_k}x{_n}", (65669, _k, _n), ("resident",), ("bwd",), kernel="gemm_wres_kernel<1, 1, ")
for _k, _n in ((16, 96), (24, 160)):
    _case(f"fused-walk-occ-{_k}x{_n}", (65669, _k, _n), ("rowA-fused-occ",), ("bwd",), kernel="gemm_rowA_kernel<1, 1, 0, ")
# weight gradient, general kernel: the three row splits with ragged tiles and three splits
for _k, _n in ((16, 36), (48, 100), (100, 164)):
    _case(f"wgrad-general-{_k}x{_n}", (600, _k, _n), ("rowA",), ("bwd_weight", "bwd", "bwd_bn"), kernel="gemm_wgrad_kernel<")
# pitches: gap columns of inputs hold NaN, gap columns of outputs are guarded
for _s in ((130, 48, 64), (130, 64, 64), (300, 16, 96)):
    _case("pitch-%dx%dx%d" % _s, _s, ("default", "rowA", "resident", "tile", "scalar"), kernel="gemm_rowA_kernel<",
          ld=dict(x=_s[1] + 8, y=_s[2] + 12, dx=_s[1] + 4, r=_s[1] + 20))


def _wgrad_cases():
    """(K, N) within 512 at which the mirrored cost rule reaches each of the thirteen tile shapes, each also one float4 beyond a
    tile edge; M = 1, MS - 1, MS + 1, a whole number of (several) splits, and that + 1"""
    for kt, nt, inst in PWW_SHAPES:
        found = None
        for kk, nn in [(kt, nt)] + [(a, b) for a in range(kt, 513, kt) for b in range(nt, 513, nt)] + \
                      [(a, b) for a in range(4, 513, 4) for b in range(4, 513, 4)]:
            if wgrad_plan(4096, kk, nn, kk, nn, {})[1]["symbol"] == "pw_wgrad_kernel<%d, %d, %d, %d>" % inst:
                found = (kk, nn)
                break
        assert found, inst
        ms = pww_ms(kt, nt)
        whole = None
        for mm in range(8 * ms, 64 * 1024, ms):
            g = wgrad_plan(mm, found[0], found[1], found[0], found[1], {})[1]
            if g["symbol"].endswith("<%d, %d, %d, %d>" % inst) and g["splits"] >= 2 and g["last_split_rows"] == g["rows_per_split"]:
                whole = mm
                break
        assert whole, inst
        tag = "%d%d%d%d" % inst
        for mm in (1, ms - 1, ms + 1, whole, whole + 1):
            _case(f"wgrad-{tag}-m{mm}", (mm,) + found, ("default",), ("bwd_weight",), kernel="pw_wgrad_kernel<%d, %d, %d, %d>" % inst)
        for mm in (ms + 1, whole + 1):
            _case(f"wgrad-{tag}-edge-m{mm}", (mm, found[0] + 4, found[1] + 4), ("default",), ("bwd_weight",), kernel="pw_wgrad_kernel<")


_wgrad_cases()

# the unaligned fall-backs (product behaviour, not a switch): the forward y, the input gradient's dx and residual offset by one float
# or at an odd pitch; ssdseg_pwconv_bwd_bn with such a dx
UNALIGNED = {"unaligned-130x16x96": ("fwd",), "unaligned-65665x16x96": ("fwd",), "unaligned-130x96x24": ("bwd_data", "bwd_bn"),
             "unaligned-65665x96x16": ("bwd_data", "bwd_bn")}
for _name, _entries in UNALIGNED.items():
    _case(_name, tuple(int(v) for v in _name.split("-")[1].split("x")), ("default", "rowA"), _entries, kernel="gemm_rowA_kernel<")
# ssdseg_pwconv_fwd_wt with a copy from ssdseg_transpose_batch: three the tile GEMM takes, one it refuses
TRANSPOSED = [("tile-k72", "tile"), ("tcols192", "tile-big"), ("tcols260", "tile-32"), ("tile-k60", "tile")]


def shape_of(name):
    return CASES[name]["shape"]


def settings_of(name):
    return CASES[name]["settings"]


def pitches(name):
    """-> dict(x, y, dx, r): row pitches of the input (and the BatchNorm raw input), of y / g / yraw, of dx, of the residual"""
    m, k, n = shape_of(name)
    return CASES[name]["ld"] or dict(x=k, y=n, dx=k, r=k)


# ------------------------------------------------------------------------------------------------------------ the forms
# A view is "plain" | "identity" or the activation code of an affine / BatchNorm-backward view.
# forward: (input view, stats); input gradient: (gradient view, residual, accumulate); weight gradient: (input view, gradient view);
# both: (input view, gradient view, residual, accumulate); fused BatchNorm: (input view, gradient view)
FWD_FORMS = [("plain", True), ("plain", False)] + [(a, a != O.ACT_RELU) for a in ACTS]
DATA_FORMS = [(O.ACT_RELU6, r, a) for r in (0, 1) for a in (0, 1)] + [("identity", 0, 0), ("identity", 1, 1), (O.ACT_NONE, 1, 0),
                                                                         (O.ACT_RELU, 0, 1), (O.ACT_ZERO, 0, 0)]
WEIGHT_FORMS = [("plain", "identity"), ("plain", O.ACT_RELU6), (O.ACT_RELU6, O.ACT_RELU6), (O.ACT_NONE, O.ACT_RELU), (O.ACT_RELU, O.ACT_NONE),
                (O.ACT_ZERO, O.ACT_RELU6), (O.ACT_RELU6, O.ACT_ZERO), (O.ACT_RELU6, "identity")]
BOTH_FORMS = [(O.ACT_RELU6, O.ACT_RELU6, r, a) for r in (0, 1) for a in (0, 1)] + \
             [("plain", "identity", 0, 0), (O.ACT_NONE, O.ACT_RELU, 1, 0), (O.ACT_RELU, O.ACT_NONE, 0, 1), (O.ACT_ZERO, O.ACT_RELU6, 0, 0),
              (O.ACT_RELU6, O.ACT_ZERO, 1, 1), (O.ACT_RELU6, "identity", 0, 0)]
BN_FORMS = [(O.ACT_RELU6, O.ACT_RELU6), (O.ACT_RELU, "identity"), (O.ACT_NONE, O.ACT_RELU), (O.ACT_ZERO, O.ACT_RELU6), (O.ACT_RELU6, O.ACT_NONE)]
LARGE_FORMS = dict(fwd=[(O.ACT_RELU6, True)], bwd_data=[(O.ACT_RELU6, 1, 1)], bwd_weight=[(O.ACT_RELU6, O.ACT_RELU6)],
                   bwd=[(O.ACT_RELU6, O.ACT_RELU6, 1, 0)], bwd_bn=[(O.ACT_RELU6, O.ACT_RELU6)])
SMALL_FORMS = dict(fwd=FWD_FORMS, bwd_data=DATA_FORMS, bwd_weight=WEIGHT_FORMS, bwd=BOTH_FORMS, bwd_bn=BN_FORMS)


def forms_of(name, entry):
    if entry not in CASES[name]["entries"]:
        return []
    return (LARGE_FORMS if CASES[name]["forms"] == "large" else SMALL_FORMS)[entry]


def form_name(form):
    return "+".join(ACT_NAMES.get(f, str(f)) if not isinstance(f, (bool, str)) else str(f) for f in form)


# ---------------------------------------------------------------------------------------------------- lattice inputs
# (scale, shift) per channel, in turn: pre-activations on both thresholds, both signs of the scale
PARAMS = [(1, 0), (2, 2), (-1, 1), (1, 4), (2, -1), (-2, 2), (2, -2), (4, 6)]
LATTICE = {   # mode: (denominator of x / g / yraw / shifts / k / mean, of the weights, largest numerator of x, of w, one value in ... kept)
    "fine": (4, 8, 8, 3, 1),
    "coarse": (1, 2, 2, 2, 1),
    "thin": (1, 2, 2, 1, 4),
    "sparse": (1, 2, 2, 1, 8),
}
MODES = ("fine", "coarse", "thin", "sparse")


class Case:
    pass


def _build(name, mode):
    m, kk, n = shape_of(name)
    xd, wd, xmax, wmax, keep = LATTICE[mode]
    rng = seeded(*[ord(ch) for ch in name])
    k = Case()
    k.name, k.shape, k.mode, k.xd, k.wd, k.ld = name, (m, kk, n), mode, xd, wd, pitches(name)

    def grid(shape, top, den):
        return (rng.integers(-top, top + 1, shape) / den).astype(F32)

    def thin(a):
        return (a * (rng.integers(0, keep, a.shape) == 0)).astype(F32) if keep > 1 else a

    gmax = 2 if mode == "sparse" else max(xmax // 2, 1)
    k.x = thin(grid((m, kk), xmax, xd))
    k.w = grid((kk, n), wmax, wd)
    k.g = thin(grid((m, n), gmax, xd))
    k.yraw = grid((m, n), xmax, xd)
    k.base = thin(grid((m, kk), gmax, xd))
    k.res = thin(grid((m, kk), gmax, xd))
    # the last row, the last float4 of the reduction and the last column carry non-zero terms in every product
    k.x[-1, -1] = k.x[0, -1] = k.x[-1, 0] = F32(1)
    k.g[-1, -1] = k.g[0, -1] = k.g[-1, 0] = F32(1)
    k.w[-1, -1] = k.w[0, -1] = k.w[-1, 0] = F32(1.0 / wd)
    noshift = mode == "sparse"
    par = np.array(PARAMS, np.float64)
    ci, co = np.arange(kk), np.arange(n)
    k.scale = par[(ci + 1) % 8, 0].astype(F32)
    k.shift = (par[(ci + 1) % 8, 1] * (0 if noshift else 1)).astype(F32)
    k.gscale = par[(co * 3 + 2) % 8, 0].astype(F32)
    k.gshift = (par[(co * 3 + 2) % 8, 1] * (0 if noshift else 1)).astype(F32)
    k.k1 = (((co * 5) % 3 - 1) / xd * (0 if noshift else 1)).astype(F32)
    k.k0 = (((co * 7) % 5 - 2) / xd * (0 if noshift else 1)).astype(F32)
    k.mean = (((ci * 3) % 5 - 2) / xd).astype(F32)
    k.invstd = np.array([1.0, 0.5, 2.0] if mode == "fine" else [1.0, 0.5, 1.0], F32)[ci % 3]
    k._own = {}
    return k


@functools.lru_cache(maxsize=None)
def mode_of(name):
    """the finest lattice whose every budget is below 2^24 (65,000 rows and more: sparse)"""
    if shape_of(name)[0] >= 65000:
        return "sparse"
    for mode in MODES:
        if max(budget(_build(name, mode)).values()) < EXACT:
            return mode
    raise AssertionError(f"{name}: no lattice keeps its reductions below 2^24")


@functools.lru_cache(maxsize=2)
def lattice_case(name):
    return _build(name, mode_of(name))


# -------------------------------------------------------------------------------------------------------- the reference
def in_view(k, view, dt=np.float64, nonstrict=False):
    """-> (activated input a, derivative mask of the producer's activation at its pre-activation)"""
    x = k.x.astype(dt)
    if view == "plain":
        return x, np.ones_like(x)
    z = x * k.scale.astype(dt) + k.shift.astype(dt)
    return O.act_fwd(z, view), (_loose_mask(z, view) if nonstrict else O.act_mask(z, view))


def _loose_mask(z, act):
    """the wrong convention: thresholds counted as inside"""
    if act == O.ACT_RELU:
        return (z >= 0).astype(z.dtype)
    if act == O.ACT_RELU6:
        return ((z >= 0) & (z <= 6)).astype(z.dtype)
    return O.act_mask(z, act)


def own_y(k, view):
    """the conv's own forward output under `view`, as float32: what ssdseg_pwconv_bwd's gradient view carries"""
    if view not in k._own:
        k._own[view] = (in_view(k, view)[0] @ k.w.astype(np.float64)).astype(F32)
    return k._own[view]


def g_view(k, gview, dt=np.float64, y=None, nonstrict=False):
    g = k.g.astype(dt)
    if gview == "identity":
        return g
    y = (k.yraw if y is None else y).astype(dt)
    s, t = k.gscale.astype(dt), k.gshift.astype(dt)
    z = s * y + t
    mk = _loose_mask(z, gview) if nonstrict else O.act_mask(z, gview)
    return s * mk * g + (k.k1.astype(dt) * y + k.k0.astype(dt))


def ref_fwd(k, view, dt=np.float64):
    """-> (y, per-column sum of y, per-column sum of y^2)"""
    a, _ = in_view(k, view, dt)
    y = a @ k.w.astype(dt)
    return y, y.sum(axis=0), (y * y).sum(axis=0)


def ref_dx(k, gview, residual=0, accumulate=0, dt=np.float64, y=None, **wrong):
    dx = g_view(k, gview, dt, y, nonstrict=wrong.get("gview_nonstrict", False)) @ k.w.astype(dt).T
    if residual:
        dx = dx + k.res.astype(dt)
    if accumulate:
        dx = dx + k.base.astype(dt)
    return dx


def ref_dw(k, view, gview, dt=np.float64, y=None):
    return in_view(k, view, dt)[0].T @ g_view(k, gview, dt, y)


def ref_bn(k, view, gview, dt=np.float64, **wrong):
    """ssdseg_pwconv_bwd_bn -> (dx, dW, dgamma, dbeta, k1, k0, (bound of k1, of k0))"""
    m = k.shape[0]
    dx = ref_dx(k, gview, 0, 0, dt, **wrong)
    _, mask = in_view(k, view, dt, nonstrict=wrong.get("view_nonstrict", False))
    mg = dx * mask
    xhat = (k.x.astype(dt) - k.mean.astype(dt)) * k.invstd.astype(dt)
    dbeta, dgamma = mg.sum(axis=0), (mg * xhat).sum(axis=0)
    sc, istd, mu = (v.astype(np.float64) for v in (k.scale, k.invstd, k.mean))
    dg64, db64 = dgamma.astype(np.float64), dbeta.astype(np.float64)
    k1 = -sc * dg64 * istd / m
    k0 = sc * (dg64 * istd * mu - db64) / m
    kbound = (U * np.abs(k1) + 2.0 ** -50 * np.abs(sc * dg64 * istd) / m,
              U * np.abs(k0) + 2.0 ** -50 * np.abs(sc) * (np.abs(dg64 * istd * mu) + np.abs(db64)) / m)
    return dx, ref_dw(k, view, gview, dt), dgamma, dbeta, k1, k0, kbound


def budget(k):
    """sum of the absolute terms of every reduction, in units of the result's lattice; < 2^24 = every partial sum in any order, fused
    or not, is exact.  K terms for y, N for dx, M for dW, M for each statistics column and each fused sum (sumsq in units of the
    squared lattice).  The statistics over the actual y of every input view; the backward over the worst view of each side (no
    clamp, every mask 1), residual and accumulation base included, with the stored yraw and with the conv's own output in the
    gradient view (ssdseg_pwconv_bwd), whose lattice is finer by the weights' denominator"""
    m, kk, n = k.shape
    xd, wd = float(k.xd), float(k.wd)
    x = np.abs(k.x.astype(np.float64))
    a = np.maximum(x, x * np.abs(k.scale) + np.abs(k.shift.astype(np.float64)))
    wa = np.abs(k.w.astype(np.float64))
    ua, uw = 1 / xd, 1 / wd
    yabs = a @ wa
    out = {"y": yabs.max() / (ua * uw), "y*y": (yabs * yabs).max() / (ua * uw) ** 2}
    ssum = ssq = 0.0
    for view in ("plain",) + ACTS:
        yv = ref_fwd(k, view)[0]
        ssum, ssq = max(ssum, np.abs(yv).sum(axis=0).max()), max(ssq, (yv * yv).sum(axis=0).max())
    out["sum"], out["sumsq"] = ssum / (ua * uw), ssq / (ua * uw) ** 2
    xhat = (x + np.abs(k.mean)) * k.invstd
    uhat = 1 / (2 * xd)
    for tag, y, uy in (("", np.abs(k.yraw.astype(np.float64)), ua), ("-own", yabs, ua * uw)):
        udy = ua * uy
        dy = np.abs(k.gscale * k.g.astype(np.float64)) + np.abs(k.k1 * y) + np.abs(k.k0.astype(np.float64))
        dxabs = dy @ wa.T + np.abs(k.res) + np.abs(k.base)
        out["dy" + tag] = dy.max() / udy
        out["dx" + tag] = dxabs.max() / (udy * uw)
        out["dW" + tag] = (a.T @ dy).max() / (ua * udy)
        if not tag:
            out["dbeta"] = dxabs.sum(axis=0).max() / (udy * uw)
            out["dgamma"] = (dxabs * xhat).sum(axis=0).max() / (udy * uw * uhat)
    return out


# ------------------------------------------------------------------------------------------------------ the normal family
NORMAL_CASES = ["rows129-16x96", "rows257-64x64", "red-k36", "red-n68", "tile-k104", "tile-n72", "cols164", "cols-k100", "tcols260",
                "grid42-257x200", "fused-129x28x100", "fused-640x32x192", "wgrad-general-48x100", "pitch-300x16x96"]
BAND = 1e-4


def _off_thresholds(v, s, t):
    z = v.astype(np.float64) * s + t
    near = (np.abs(z) < BAND) | (np.abs(z - 6) < BAND)
    return np.where(near, v + F32(0.05), v).astype(F32)


@functools.lru_cache(maxsize=2)
def normal_case(name):
    m, kk, n = shape_of(name)
    rng = seeded(7, *[ord(ch) for ch in name])
    k = Case()
    k.name, k.shape, k.mode, k.ld = name, (m, kk, n), "normal", pitches(name)
    k.scale = (rng.uniform(0.5, 1.5, kk) * rng.choice([-1.0, 1.0], kk, p=[0.25, 0.75])).astype(F32)
    k.shift = rng.uniform(-1, 3, kk).astype(F32)
    k.gscale = rng.uniform(0.5, 1.5, n).astype(F32)
    k.gshift = rng.uniform(-1, 3, n).astype(F32)
    k.x = _off_thresholds(rng.normal(0, 2, (m, kk)).astype(F32), k.scale, k.shift)
    k.yraw = _off_thresholds(rng.normal(0, 2, (m, n)).astype(F32), k.gscale, k.gshift)
    k.w = rng.normal(0, 0.3, (kk, n)).astype(F32)
    k.g = rng.normal(0, 2, (m, n)).astype(F32)
    k.base = rng.normal(0, 2, (m, kk)).astype(F32)
    k.res = rng.normal(0, 2, (m, kk)).astype(F32)
    k.k1 = rng.normal(0, 0.1, n).astype(F32)
    k.k0 = rng.normal(0, 0.1, n).astype(F32)
    k.mean = k.x.mean(axis=0, dtype=np.float64).astype(F32)
    k.invstd = (1.0 / np.sqrt(k.x.var(axis=0, dtype=np.float64) + 1e-3)).astype(F32)
    k._own = {}
    return k


def normal_bounds(k, view, gview, residual=0, accumulate=0):
    """any-order per-element and per-column bounds of one form of a normal case (derivations: tests/test_gpu_pw_edges.py)"""
    m, kk, n = k.shape
    x = k.x.astype(np.float64)
    za = np.abs(x) if view == "plain" else np.abs(x * k.scale) + np.abs(k.shift.astype(np.float64))      # A = |s x| + |t| >= |z|, |a|
    a, mask = in_view(k, view)
    wa = np.abs(k.w.astype(np.float64))
    y, _, _ = ref_fwd(k, view)
    y_b = (gamma(kk + 1) + U) * (za @ wa)
    sum_b = gamma(m + 1) * np.abs(y).sum(axis=0) + y_b.sum(axis=0)
    sq_b = gamma(m + 2) * (y * y).sum(axis=0) + (2 * np.abs(y) * y_b + y_b * y_b).sum(axis=0)
    g, yr = k.g.astype(np.float64), k.yraw.astype(np.float64)
    dabs = np.abs(g) if gview == "identity" else np.abs(k.gscale * g) + np.abs(k.k1 * yr) + np.abs(k.k0.astype(np.float64))
    dx = ref_dx(k, gview, residual, accumulate)
    dx_b = (gamma(n + 1) + 2 * U) * (dabs @ wa.T)
    run = np.abs(ref_dx(k, gview))
    for on, term in ((residual, k.res), (accumulate, k.base)):
        if on:
            run = run + np.abs(term.astype(np.float64))
            dx_b = dx_b + U * (run + dx_b)
    dw = ref_dw(k, view, gview)
    dw_b = (gamma(m + 2) + 3 * U) * (za.T @ dabs) + U * np.abs(dw)
    xhat = np.abs((x - k.mean) * k.invstd)
    mdx = np.abs(dx * mask)
    dbeta_b = gamma(m + 1) * mdx.sum(axis=0) + (dx_b * mask).sum(axis=0) + U * np.abs((dx * mask).sum(axis=0))
    dgamma_b = (gamma(m + 2) + 2 * U) * (mdx * xhat).sum(axis=0) + (dx_b * mask * xhat).sum(axis=0) + \
        U * np.abs((dx * mask * (x - k.mean) * k.invstd).sum(axis=0))
    return dict(y=y_b, sum=sum_b, sumsq=sq_b, dx=dx_b, dW=dw_b, dbeta=dbeta_b, dgamma=dgamma_b)


# ------------------------------------------------------------------------------------------- the launches a form must make
def expected_launches(name, setting, entry, form, aligned=True):
    """-> ({kernel symbol: launches}, geometry) of one form of one entry point of a case under a setting, by the mirror"""
    m, k, n = shape_of(name)
    ld, env = pitches(name), SETTINGS[setting]
    if entry == "fwd":
        return plan_fwd(m, k, n, ld["x"], env, aligned=aligned, stats=form[1])
    if entry == "bwd_data":
        return plan_bwd_data(m, k, n, ld["y"], env, form[0] != "identity", bool(form[1] or form[2]), aligned)
    if entry == "bwd_weight":
        return wgrad_plan(m, k, n, ld["x"], ld["y"], env)
    if entry == "bwd":
        return plan_bwd(m, k, n, ld["x"], ld["y"], env, form[1] != "identity", bool(form[2] or form[3]), aligned)
    return plan_bwd_bn(m, k, n, ld["x"], ld["y"], env, form[1] != "identity", aligned)


def planned_symbols():
    """every kernel symbol the mirror expects over all cases, settings, entry points and forms"""
    seen = set()
    for name in CASES:
        for setting in settings_of(name):
            for entry in CASES[name]["entries"]:
                for form in forms_of(name, entry):
                    seen.update(expected_launches(name, setting, entry, form)[0])
    return seen


# what the suite must reach (the issue's coverage list), as predicates over the set of symbols
def coverage_gaps(seen):
    want = []
    for occ in (0, 1):
        want.append((f"fused rowA form, OCC {occ}", lambda s, o=occ: s.startswith("gemm_rowA_kernel<1, 1, 0, ") and s.endswith(f", 0, {o}>")
                     and not s.startswith("gemm_rowA_kernel<1, 1, 0, 0,")))
    for nt in (2, 3, 4):
        want.append((f"resident fused form NT {nt}", lambda s, t=nt: s == f"gemm_wres_kernel<1, 1, {t}>"))
    for ep in (1, 2):
        want.append((f"OCC rowA EP {ep} WN <= 3", lambda s, e=ep: any(s.startswith(f"gemm_rowA_kernel<{w}, ") for w in (1, 2, 3)) and s.endswith(f", 0, 0, {e}, 1>")))
        want.append((f"OCC rowA EP {ep} WN >= 4", lambda s, e=ep: any(s.startswith(f"gemm_rowA_kernel<{w}, ") for w in (4, 5)) and s.endswith(f", 0, 0, {e}, 1>")))
    for wn in (2, 4, 5, 6, 8):
        want.append((f"eight-wave tile GEMM WN {wn}", lambda s, w=wn: s.startswith(f"pw_tile_kernel<8, {w}, ") and s.count(",") == 2))
    want.append(("4 x 2 grid, three tiles", lambda s: s == "pw_tile_kernel<8, 3, 1, 2>"))
    want.append(("4 x 2 grid, four tiles", lambda s: s == "pw_tile_kernel<8, 4, 1, 2>"))
    for _, _, inst in PWW_SHAPES:
        want.append(("row-naming weight gradient %s" % (inst,), lambda s, i=inst: s == "pw_wgrad_kernel<%d, %d, %d, %d>" % i))
    for wi, wr in ((1, 4), (2, 2), (4, 1)):
        want.append((f"general weight gradient <{wi}, {wr}, .>", lambda s, a=wi, b=wr: s.startswith(f"gemm_wgrad_kernel<{a}, {b}, ")))
    return [what for what, pred in want if not any(pred(s) for s in seen)]
