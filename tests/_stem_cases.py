"""Named edge cases, the float64 reference, bounds and a mirror of the host geometry for the stem conv and the 3x3 / 2 max-pool: plain NumPy.

The entry points are ssdseg_stem_conv_parts / _fwd / _bwd_weight (csrc/stem.hip: stem_fwd_direct_kernel<Q>, Q = 1 .. 16; the LD == 2
loader of gemm_rowA_kernel in csrc/gemm.hip; the stem gather of gemm_wgrad_kernel in csrc/pw_wgrad.hip) and ssdseg_maxpool3x3s2_fwd /
_bwd (csrc/shuffle.hip).  tests/test_cpu_stem_cases.py vets the reference, the cases and the mirror on the CPU;
tests/test_gpu_stem_edges.py runs the kernels on the same cases.  Every builder seeds its own generator from the case's name, so the
same call gives the same arrays in both files.  Stem shapes are (n, h, w, cout), pool shapes (n, h, w, c).

The lattice family.  Pixels are integers in [0, 255] (`bytes`), [0, 15] (`nibble`) or [0, 3] (`tiny`), weights and bias multiples of
1/8 with |w| <= 1, g, yraw, the shifts, k1 and k0 multiples of 1/4, the gradient view's scales signed powers of two, and the rescale
(in_scale, in_offset) one of the power-of-two PAIRS: w . scale, offset . sum_c w, the nine-tap sum, the border subtraction and the 27
multiply-adds of the direct kernel are then float32 numbers, and so is fmaf(x, scale, offset) of the implicit GEMM and of the weight
gradient.  `budget` gives, in units of each result's lattice, the sum of the absolute terms of every reduction a kernel forms; below
2^24 the float64 reference IS the float32 result in any order and the bound is 0.

The normal family.  Random bytes, N(0, 0.3) weights, the production rescale (1 / 127.5 as the float32 the C ABI receives, -1);
any-order bounds with U = 2^-24, gamma(L) = L U / (1 - L U) (derivations: the docstring of tests/test_gpu_stem_edges.py).

The mirror is of the GEOMETRY the cases are named after: TF SAME for k = 3, s = 2, ssdseg_stem_direct_eligible / _blocks, QP and PPB
per Q, the rows of ssdseg_stem_conv_parts, the row tiles a block of the implicit GEMM walks, and the split rule of wgrad_run at K = 27.
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
NUM_CUS = 256                   # the MI355X; the GPU file passes the device's own count
# every switch the stem and the pool read per call, and (the implicit GEMM and the weight gradient are pointwise kernels) the pointwise ones
STEM_VARS = ("SSDSEG_STEM_DIRECT", "SSDSEG_MAXPOOL_BWD") + PW.PW_VARS
FORM_ENV = {"direct": {}, "gemm": {"SSDSEG_STEM_DIRECT": "0"}}
PAIRS = ((2.0 ** -7, -1.0), (2.0 ** -2, -0.5), (1.0, 0.0), (2.0 ** -7, 0.0))         # (in_scale, in_offset) of the lattice family
NORMAL_PAIR = (float(F32(1.0 / 127.5)), -1.0)


def seeded(*key):
    return np.random.default_rng([1993, 404] + [int(k) for k in key])


# ================================================================================================= mirror of the host geometry
MAX_BLOCKS, BM, WG_ROWS = 2048, 128, 64


def same_geometry(h, w):
    """stem_geometry / pool_geom: TF SAME, kernel 3, stride 2 -> (ho, wo, pt, pl)"""
    return (h + 1) // 2, (w + 1) // 2, h % 2, w % 2


def direct_eligible(cout):
    return cout % 4 == 0 and 4 <= cout <= 64


def direct_blocks(n, h):
    return min(n * ((h + 1) // 2), MAX_BLOCKS)


def qp_of(q):
    return (q + 3) // 4 * 4


def ppb_of(q):
    return 256 // qp_of(q)


def takes_direct(env, n, h, w, cout):
    return env.get("SSDSEG_STEM_DIRECT", "")[:1] != "0" and direct_eligible(cout) and n * h * w * 12 < (1 << 31)


def gemm_rows(n, h, w, cout):
    ho, wo, _, _ = same_geometry(h, w)
    return PW.rowA_grid_y(n * ho * wo, cout, {})


def gemm_walk(n, h, w, cout):
    """row tiles of 128 a block of the implicit GEMM works on in turn (rowA_grid_y_wn's `per`)"""
    ho, wo, _, _ = same_geometry(h, w)
    return cdiv(cdiv(n * ho * wo, BM), gemm_rows(n, h, w, cout))


def table_rows(n, h, w, cout):
    """== ssdseg_stem_conv_parts: the larger of the two forward kernels' row counts"""
    return max(gemm_rows(n, h, w, cout), direct_blocks(n, h) if direct_eligible(cout) else 0)


def launch_rows(env, n, h, w, cout):
    return direct_blocks(n, h) if takes_direct(env, n, h, w, cout) else gemm_rows(n, h, w, cout)


def wgrad_plan(m, cout, num_cus=NUM_CUS):
    """wgrad_run at K = 27 (never the row-naming kernel: K % 4 != 0): wi = 1, 64-row steps, max_splits, the traffic cap, wn <= 3, splits
    dealt by steps -> dict(wn, jtiles, steps, splits, sps, rows_per_split, last_rows, symbol)"""
    k = 27
    steps = cdiv(m, WG_ROWS)
    max_splits = cdiv(steps, 4)
    cap = int(float(m) * (k + cout) * 0.5 / (float(k) * cout))
    if max_splits > cap:
        max_splits = max(cap, 1)
    wn = min(PW.pick_wn(cout, max_splits), 3)
    jtiles = cdiv(cout, 32 * wn)
    want = cdiv((4 if m >= PW.ROWA_OCC_ROWS else 2) * num_cus, jtiles)
    splits = min(max(1, min(want, max_splits)), 65535)
    sps = cdiv(steps, splits)
    splits = cdiv(steps, sps)
    rps = sps * WG_ROWS
    return dict(wn=wn, jtiles=jtiles, steps=steps, splits=splits, sps=sps, rows_per_split=rps, last_rows=m - (splits - 1) * rps,
                symbol=f"gemm_wgrad_kernel<1, 4, {wn}> [conv3x3 tap]")        # (the registry labels every launch with conv geometry so, the stem gather included)


def smallest_m(splits, cout=4, num_cus=NUM_CUS):
    """the smallest M with that many splits whose last split is shorter than the others"""
    for m in range(1, 1 << 14):
        p = wgrad_plan(m, cout, num_cus)
        if p["splits"] == splits and p["last_rows"] < p["rows_per_split"]:
            return m
    raise AssertionError(splits)


def fwd_kernel(form, n, h, w, cout):
    """a regular expression of the forward kernel symbol (timing registry spelling)"""
    if takes_direct(FORM_ENV[form], n, h, w, cout):
        return r"^stem_fwd_direct_kernel<%d>$" % (cout // 4)
    ho, wo, _, _ = same_geometry(h, w)
    return r"^gemm_rowA_kernel<%d, 0, 2, 0, 0, \d>$" % PW.rowA_wn(n * ho * wo, cout, {})


def reaches(launches, pattern):
    return any(re.search(pattern, s) for s in launches)


# ============================================================================================================ the stem cases
# name: dict(shape, forms ("direct" / "gemm": the setting, not the kernel -- cout > 64 runs the GEMM under both), variants
# ("stats", "bias", "none"), pairs (indices of PAIRS), wgrad (run the weight gradient too), why)
CASES = {}
ALL_PAIRS = (0, 1, 2, 3)


def _case(name, shape, forms, variants=("stats", "bias"), pairs=ALL_PAIRS, fwd=True, wgrad=False, why=""):
    assert name not in CASES, name
    CASES[name] = dict(shape=tuple(shape), forms=tuple(forms), variants=tuple(variants), pairs=tuple(pairs), fwd=fwd, wgrad=wgrad, why=why)


for _q in range(1, 17):
    _case(f"inst-{_q}", (2, 5, 7, 4 * _q), ("direct",), ("stats", "bias", "none"), why="every instantiation; idle lanes; two images")
for _h in (1, 2, 3, 4):
    for _w in (1, 2, 3, 4):
        _case(f"pad-{_h}x{_w}", (1, _h, _w, 8), ("direct", "gemm"), why="pad pairs; every corner and edge pixel's removed-offset set")
PPT = {}                                        # name: (PPB, wo)
for _cout in (16, 32, 48, 64):
    _ppb = ppb_of(_cout // 4)
    for _wo in (_ppb - 1, _ppb, _ppb + 1, 2 * _ppb, 2 * _ppb + 1):
        PPT[f"ppt-{_cout}-{_wo}"] = (_ppb, _wo)
        _case(f"ppt-{_cout}-{_wo}", (1, 2, 2 * _wo - _wo % 2, _cout), ("direct",), ("stats",), why="the second pixel of a thread; a second trip")
_case("rows-2050-8", (1025, 3, 1, 8), ("direct",), ("stats",), pairs=(1,), why="2,050 output rows on 2,048 blocks")
_case("rows-2050-24", (1025, 4, 2, 24), ("direct",), ("stats",), pairs=(1,), why="2,050 output rows on 2,048 blocks, idle lanes")
_case("stats-40x40", (1, 40, 40, 4), ("direct", "gemm"), ("stats",), why="20 direct rows, 4 GEMM rows: the GEMM form's tail is zero")
_case("stats-3x3-64", (2, 3, 3, 64), ("gemm", "direct"), ("stats",), why="4 direct rows, 1 GEMM row")
for _cout in (68, 100):
    _case(f"fallback-{_cout}", (1, 5, 7, _cout), ("direct",), why="cout > 64: the implicit GEMM whatever the switch says")
for _m, _shape in ((1, (1, 1, 1, 8)), (127, (1, 2, 254, 8)), (128, (1, 2, 256, 8)), (129, (1, 2, 258, 8))):
    _case(f"gemm-rows{_m}", _shape, ("gemm",), why="ragged 128-row tiles; the K = 27 tail of the 32-wide step")
_case("gemm-3img", (3, 11, 13, 12), ("gemm",), why="three 42-pixel images in one 128-row tile")
for _cout in (4, 12, 36, 68, 100, 164):
    _case(f"gemm-cout{_cout}", (2, 5, 7, _cout), ("gemm",), why="every column-tile width and two column tiles; bias in the epilogue")
GEMM_WN = {68: 3, 132: 5}         # cout: the column-tile width once 512 blocks fill the chip; below that rowA_wn picks 32-wide tiles (the cases above run 1 .. 6 of them)
for _cout in GEMM_WN:
    _case(f"gemm-wn-c{_cout}", (1, 512, 512, _cout), ("gemm",), ("stats",), pairs=(1,), why="65,536 rows: a wider column tile")
BIG = "gemm-walk"
_case(BIG, (1, 1026, 1026, 4), ("gemm",), ("stats",), pairs=(1,), why="2,057 row tiles on 686 blocks: a block walks three and adds to its row")
WG_M = {1: (1, 1, 1), 63: (1, 13, 17), 64: (1, 16, 16), 65: (1, 10, 25), 257: (1, 1, 513), 513: (3, 17, 37)}      # n ho wo: (n, h, w)
WG_COUT = (4, 24, 32, 36, 64, 68, 100)
for _m, _nhw in WG_M.items():
    for _cout in WG_COUT:
        _case(f"wg-m{_m}-c{_cout}", _nhw + (_cout,), (), (), pairs=((0, 1) if _m in (65, 513) else (1,)), fwd=False, wgrad=True, why="weight gradient: steps, splits, columns")
WG_WIDE = {64: 2, 100: 3}                      # cout: wn once 512 splits fill the chip (100: two column tiles of 96)
for _cout in WG_WIDE:
    _case(f"wg-wide-c{_cout}", (1, 723, 724, _cout), (), (), pairs=(1,), fwd=False, wgrad=True, why="131,044 rows: wn = 2, 3 and two column tiles of 96")
WGRAD_FORMS = (("identity", True), (O.ACT_RELU6, False))       # (gradient view, dbias)


def shape_of(name):
    return CASES[name]["shape"]


def m_of(name):
    n, h, w, _ = shape_of(name)
    ho, wo, _, _ = same_geometry(h, w)
    return n * ho * wo


# ---------------------------------------------------------------------------------------------------- lattice inputs
PARAMS = PW.PARAMS      # (scale, shift) per channel of the gradient view: pre-activations on both thresholds, both signs of the scale
LATTICE = {             # mode: (largest pixel, largest numerator of w and bias over 8, of g over 4, of yraw over 4)
    "bytes": (255, 8, 4, 8),
    "nibble": (15, 4, 2, 8),
    "tiny": (3, 1, 1, 2),
}
MODES = ("bytes", "nibble", "tiny")


class Case:
    pass


def _build(name, mode):
    n, h, w, cout = shape_of(name)
    ho, wo, pt, pl = same_geometry(h, w)
    xmax, wtop, gtop, ytop = LATTICE[mode]
    rng = seeded(*[ord(ch) for ch in name])
    k = Case()
    k.name, k.shape, k.mode, k.geo = name, (n, h, w, cout), mode, (ho, wo, pt, pl)
    k.x = rng.integers(0, xmax + 1, (n, h, w, 3)).astype(F32)
    k.w = (rng.integers(-wtop, wtop + 1, (3, 3, 3, cout)) / 8).astype(F32)
    k.b = (rng.integers(-wtop, wtop + 1, cout) / 8).astype(F32)
    k.g = (rng.integers(-gtop, gtop + 1, (n, ho, wo, cout)) / 4).astype(F32)
    k.yraw = (rng.integers(-ytop, ytop + 1, (n, ho, wo, cout)) / 4).astype(F32)
    # the corners of every image are bright, every tap of the first and last column carries a non-zero offset term, the corners of the
    # gradient are non-zero
    k.x[:, 0, 0] = k.x[:, -1, -1] = k.x[:, 0, -1] = k.x[:, -1, 0] = F32(xmax)
    k.w[:, :, :, -1] = np.array([1, 1, -1], F32) / 8
    k.w[:, :, :, 0] = np.array([1, -1, 1], F32) / 8
    k.b[0] = k.b[-1] = F32(1 / 8)
    for a in (k.g, k.yraw):
        a[:, 0, 0, -1] = a[:, -1, -1, -1] = a[:, 0, -1, 0] = a[:, -1, 0, 0] = F32(0.25)
    par = np.array(PARAMS, np.float64)
    co = np.arange(cout)
    k.gscale = par[(co * 3 + 2) % 8, 0].astype(F32)
    k.gshift = par[(co * 3 + 2) % 8, 1].astype(F32)
    k.k1 = (((co * 5) % 3 - 1) / 4).astype(F32)
    k.k0 = (((co * 7) % 5 - 2) / 4).astype(F32)
    k._refs = {}
    return k


MUST_HOLD = ("y", "sum", "dW", "dbias")


def holds(k):
    return all(max(budget(k, PAIRS[i])[q] for q in MUST_HOLD) < EXACT for i in CASES[k.name]["pairs"])


@functools.lru_cache(maxsize=None)
def mode_of(name):
    """the widest pixel range whose every budget (sumsq apart: the GPU file bounds it where it does not hold) is below 2^24 under every
    rescale pair of the case; 65,000 output pixels and more: tiny"""
    for mode in (MODES if m_of(name) < 65000 else ("tiny",)):
        if holds(_build(name, mode)):
            return mode
    raise AssertionError(f"{name}: no lattice keeps its reductions below 2^24")


@functools.lru_cache(maxsize=2)
def lattice_case(name):
    return _build(name, mode_of(name))


# -------------------------------------------------------------------------------------------------------- the reference
def rescaled(k, pair, dt=np.float64):
    return O.rescale(k.x.astype(dt), dt(pair[0]), dt(pair[1]))


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


def ref_fwd(k, pair, bias=False, dt=np.float64):
    def make():
        return O.conv2d_fwd(rescaled(k, pair, dt), k.w.astype(dt), 2, 1, k.b.astype(dt) if bias else None)
    return _ref(k, ("fwd", pair, bias, dt), make)


def ref_bwd(k, pair, gview, dt=np.float64):
    """-> (dW, dbias)"""
    return _ref(k, ("bwd", pair, gview, dt), lambda: O.conv2d_bwd(rescaled(k, pair, dt), k.w.astype(dt), g_view(k, gview, dt), 2, 1)[1:])


def gather(k, pt=None, pl=None, neighbour=False, rows=4):
    """the operand of the implicit GEMM before the rescale -> (pixels (rows * 3, n, ho, wo, 3) with 0 where nothing is read, inside (rows * 3,
    n, ho, wo): the tap lies in its image, read: the tap is read); tap = kh * 3 + kw, rows 3 = the nine taps, rows 4 = three more (what a
    28th .. 36th reduction element would read).  neighbour: a tap outside its image is read wherever the flat buffer holds a pixel there
    (the next image's row, the previous row's end)"""
    n, h, w, _ = k.shape
    ho, wo, pt0, pl0 = k.geo
    pt, pl = pt0 if pt is None else pt, pl0 if pl is None else pl
    flat = k.x.astype(np.float64).reshape(n * h * w, 3)
    img = np.arange(n)[:, None, None]
    px, inside, read = [], [], []
    for kh in range(rows):
        for kw in range(3):
            iy, ix = (2 * np.arange(ho) - pt + kh)[None, :, None], (2 * np.arange(wo) - pl + kw)[None, None, :]
            ok = np.broadcast_to((iy >= 0) & (iy < h) & (ix >= 0) & (ix < w), (n, ho, wo))
            at = (img * h + iy) * w + ix
            rd = (at >= 0) & (at < n * h * w) if neighbour else ok
            px.append(np.where(rd[..., None], flat[np.clip(at, 0, n * h * w - 1)], 0.0))
            inside.append(ok)
            read.append(rd)
    return np.stack(px), np.stack(inside), np.stack(read)


def by_taps(k, pair, bias=False, keep_offset=None, drop_offset=None, drop_k=None, extra_k=False, **how):
    """y the way the kernels form it: sum over valid taps of (x s + o) w, tap by tap -- with one structural error if asked for:
    keep_offset = tap: the offset term left in where that tap is padded; drop_offset = tap: removed where it is valid; drop_k: that
    reduction element left out; extra_k: a 28th taken (the pixel below the window's first column, times the weights' last row);
    pt / pl / neighbour: see `gather`"""
    s, o = pair
    px, ok, read = gather(k, **how)
    w = k.w.astype(np.float64).reshape(27, -1)
    y = np.zeros(px.shape[1:4] + (w.shape[1],))
    for tap in range(9):
        a = np.where(read[tap][..., None], px[tap] * s + o, 0.0)
        if keep_offset == tap:
            a = np.where(ok[tap][..., None], a, o)
        if drop_offset == tap:
            a = a - np.where(ok[tap][..., None], o, 0.0)
        for c in range(3):
            if drop_k != tap * 3 + c:
                y += a[..., c:c + 1] * w[tap * 3 + c]
    if extra_k:
        y += np.where(ok[9][..., None], px[9][..., :1] * s + o, 0.0) * w[26]
    return y + k.b.astype(np.float64) if bias else y


def dw_wrong(k, pair, gview, rows=None, padded_as_offset=False):
    """dW with a structural error: only the first `rows` output pixels summed; a padded tap counted as `offset`, not 0"""
    s, o = pair
    px, ok, _ = gather(k, rows=3)
    dy = g_view(k, gview).reshape(-1, k.shape[3])
    dw = np.zeros((27, k.shape[3]))
    for tap in range(9):
        a = np.where(ok[tap][..., None], px[tap] * s + o, o if padded_as_offset else 0.0).reshape(-1, 3)
        dw[tap * 3:tap * 3 + 3] = a[:rows].T @ dy[:rows]
    return dw.reshape(3, 3, 3, -1)


def abs_terms(k, pair, bias=False):
    """-> (sum |x s w| over valid taps, |o| sum_c |w| over all nine taps, the same over the padded taps, |b|), each (n, ho, wo, cout) or
    broadcastable to it: the terms the direct kernel forms"""
    s, o = pair
    wa = np.abs(k.w.astype(np.float64))
    data = O.conv2d_fwd(np.abs(k.x.astype(np.float64) * s), wa, 2, 1)
    every = abs(o) * wa.sum(axis=(0, 1, 2))
    removed = every - abs(o) * O.conv2d_fwd(np.ones(k.x.shape), wa, 2, 1)
    return data, every, np.maximum(removed, 0.0), (np.abs(k.b.astype(np.float64)) if bias else 0.0)


def a_abs(k, pair):
    return np.abs(k.x.astype(np.float64) * pair[0]) + abs(pair[1])


def d_abs(k, gview):
    g, yr = k.g.astype(np.float64), k.yraw.astype(np.float64)
    return np.abs(g) if gview == "identity" else np.abs(k.gscale * g) + np.abs(k.k1 * yr) + np.abs(k.k0.astype(np.float64))


def budget(k, pair):
    """sum of the absolute terms of every reduction a kernel forms, in units of the result's lattice; < 2^24 = every partial sum in any
    order, fused or not, is exact.  y (unit scale / 8; the offset terms and the bias are multiples of it): 27 data terms, 9 offset terms
    and the up-to-8 removed offset terms again (the direct kernel adds all nine and subtracts the padded ones), the bias -- which also
    covers the GEMM form's 27 products of |x s| + |o|.  sum y per statistics row and per column fold: n ho wo terms (sumsq in units of
    the squared lattice).  dW (unit scale / 16: fmaf(x, s, o) is a multiple of scale, the gradient view's dy of 1/16): n ho wo terms over
    the worst gradient view (every mask 1).  dbias (unit 1/4): n ho wo terms"""
    s, o = pair
    uy = s / 8
    data, every, removed, b = abs_terms(k, pair, True)
    out = {"y": (data + every + removed + b).max() / uy}
    y = ref_fwd(k, pair)
    out["sum"] = max(np.abs(y).sum(axis=(0, 1, 2)).max(), np.abs(ref_fwd(k, pair, True)).sum(axis=(0, 1, 2)).max()) / uy
    out["sumsq"] = (y * y).sum(axis=(0, 1, 2)).max() / uy ** 2
    dy = np.maximum(d_abs(k, "identity"), d_abs(k, O.ACT_RELU6))
    out["dW"] = O.conv2d_bwd(a_abs(k, pair), k.w.astype(np.float64), dy, 2, 1)[1].max() / (s / 16)
    out["dbias"] = np.abs(k.g.astype(np.float64)).sum(axis=(0, 1, 2)).max() * 4
    return out


# ------------------------------------------------------------------------------------------------------ the normal family
NORMAL_CASES = ["inst-6", "inst-8", "inst-10", "inst-16", "pad-1x1", "pad-3x4", "ppt-48-43", "ppt-16-129", "stats-40x40", "gemm-3img",
                "gemm-cout164", "fallback-100", "wg-m65-c24", "wg-m257-c36", "wg-m513-c100"]
BAND = 1e-4
# roundings of stem_fwd_direct_kernel beyond its 27 multiply-adds (csrc/stem.hip; derivation in tests/test_gpu_stem_edges.py)
DIRECT_C1 = 8 + 1 + 8      # the eight additions of wo_all (:56), bias + wo_all (:96), up to eight subtractions at a border (:102)
DIRECT_C2 = 3              # forming a term: w . scale once (:51); sum_c w twice and . offset once (:52, :54)
SECOND_ORDER = 1 + 2.0 ** -16


@functools.lru_cache(maxsize=2)
def normal_case(name):
    n, h, w, cout = shape_of(name)
    ho, wo, pt, pl = same_geometry(h, w)
    rng = seeded(7, *[ord(ch) for ch in name])
    k = Case()
    k.name, k.shape, k.mode, k.geo = name, (n, h, w, cout), "normal", (ho, wo, pt, pl)
    k.x = rng.integers(0, 256, (n, h, w, 3)).astype(F32)
    k.w = rng.normal(0, 0.3, (3, 3, 3, cout)).astype(F32)
    k.b = rng.normal(0, 0.3, cout).astype(F32)
    k.g = rng.normal(0, 1, (n, ho, wo, cout)).astype(F32)
    k.gscale = rng.uniform(0.5, 1.5, cout).astype(F32)
    k.gshift = rng.uniform(-1, 3, cout).astype(F32)
    yraw = rng.normal(0, 2, (n, ho, wo, cout)).astype(F32)
    z = yraw.astype(np.float64) * k.gscale + k.gshift
    k.yraw = np.where((np.abs(z) < BAND) | (np.abs(z - 6) < BAND), yraw + F32(0.05), yraw).astype(F32)
    k.k1 = rng.normal(0, 0.1, cout).astype(F32)
    k.k0 = rng.normal(0, 0.1, cout).astype(F32)
    k._refs = {}
    return k


def fwd_bound(k, pair, form_is_direct, bias=False):
    """per element.  direct: (gamma(27 + c1) + c2 U) T, T the absolute terms the kernel forms (`abs_terms`: the removed offset terms count
    twice), times (1 + 2^-16) for the products of two errors.  GEMM: (gamma(27 + 1) + U) sum (|x s| + |o|) |w| + U |b|"""
    if form_is_direct:
        data, every, removed, b = abs_terms(k, pair, bias)
        return (gamma(27 + DIRECT_C1) + DIRECT_C2 * U) * SECOND_ORDER * (data + every + removed + b)
    t = O.conv2d_fwd(a_abs(k, pair), np.abs(k.w.astype(np.float64)), 2, 1)
    return (gamma(27 + 1) + U) * t + (U * np.abs(k.b.astype(np.float64)) if bias else 0.0)


def stats_bounds(y, y_b):
    """-> (bound of sum y, of sum y^2) over m = n ho wo pixels from y within y_b"""
    m = y.shape[0] * y.shape[1] * y.shape[2]
    return (gamma(m + 1) * np.abs(y).sum(axis=(0, 1, 2)) + np.broadcast_to(y_b, y.shape).sum(axis=(0, 1, 2)),
            gamma(m + 2) * (y * y).sum(axis=(0, 1, 2)) + (2 * np.abs(y) * y_b + y_b * y_b).sum(axis=(0, 1, 2)))


def bwd_bounds(k, pair, gview):
    """-> (bound of dW, of dbias): gemm_wgrad_kernel's rows of the pointwise suite with A = |x s| + |o| at the valid taps; the bias
    gradient a float32 chain of at most M terms, the fold and one rounding"""
    m = m_of(k.name)
    dw, db = ref_bwd(k, pair, gview)
    dwa = O.conv2d_bwd(a_abs(k, pair), k.w.astype(np.float64), d_abs(k, gview), 2, 1)[1]
    return (gamma(m + 2) + 3 * U) * dwa + U * np.abs(dw), gamma(m + 1) * np.abs(k.g.astype(np.float64)).sum(axis=(0, 1, 2)) + U * np.abs(db)


# ============================================================================================================ the max-pool
POOL_SHAPES = [(2, _h, _w, 4) for _h in (1, 2, 3, 4, 5) for _w in (1, 2, 3, 4, 5)] + [(2, 7, 9, 24), (1, 8, 6, 116), (3, 6, 5, 232)]
POOL_VIEWS = ("plain", O.ACT_RELU, O.ACT_RELU6)
POOL_PARAMS = [(8, 3), (-4, 3), (4, 3), (-8, 3)]        # (scale, shift) per channel in turn: over a third of [-2, 2] at or below 0, at or above 6
POOL_SPECIAL = {"all-negative": (2, 5, 5, 4), "signed-zeros": (2, 5, 5, 4)}


@functools.lru_cache(maxsize=4)
def pool_case(shape, kind="regular"):
    """x and g multiples of 1/4; the last image repeats the first (the same bits are demanded of it).  all-negative: every pre-activation
    below 0 (scale 1, shift -4), so every window is a tie among all its valid cells under ReLU.  signed-zeros: nothing above zero, and
    the zeros carry either sign"""
    n, h, w, c = shape
    ho, wo, pt, pl = same_geometry(h, w)
    rng = seeded(11, n, h, w, c, len(kind))
    k = Case()
    k.shape, k.kind, k.geo = shape, kind, (ho, wo, pt, pl)
    k.x = (rng.integers(-8, 9, shape) / 4).astype(F32)
    if kind == "signed-zeros":
        mag = np.abs(k.x) * (rng.integers(0, 3, shape) == 0)
        k.x = np.where((mag == 0) & (rng.integers(0, 2, shape) == 0), F32(0.0), -mag).astype(F32)
    k.g = (rng.integers(-4, 5, (n, ho, wo, c)) / 4).astype(F32)
    k.g[k.g == 0] = F32(0.25)
    k.x[-1], k.g[-1] = k.x[0], k.g[0]
    par = np.array(POOL_PARAMS, np.float64)
    k.scale = par[np.arange(c) % 4, 0].astype(F32) if kind != "all-negative" else np.ones(c, F32)
    k.shift = par[np.arange(c) % 4, 1].astype(F32) if kind != "all-negative" else np.full(c, -4, F32)
    return k


def pool_in(k, view, dt=np.float64):
    x = k.x.astype(dt)
    return x if view == "plain" else O.act_fwd(x * k.scale.astype(dt) + k.shift.astype(dt), view)


def pool_windows(a):
    """(9, n, ho, wo, c) values with -inf at a padded cell, tap = kh * 3 + kw"""
    n, h, w, c = a.shape
    ho, wo, pt, pl = same_geometry(h, w)
    ap = np.full((n, 2 * ho + 2, 2 * wo + 2, c), -np.inf)
    ap[:, pt:pt + h, pl:pl + w] = a
    return np.stack([ap[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] for kh in range(3) for kw in range(3)])


def pool_bwd_by(a, g, winner):
    """dx with the winning tap(s) of every window named by `winner`: (9, n, ho, wo, c) of 0 / 1"""
    n, h, w, c = a.shape
    ho, wo, pt, pl = same_geometry(h, w)
    dxp = np.zeros((n, 2 * ho + 2, 2 * wo + 2, c))
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        dxp[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] += g * winner[tap]
    return dxp[:, pt:pt + h, pl:pl + w]


def one_hot(arg):
    return (np.arange(9).reshape(9, 1, 1, 1, 1) == arg[None]).astype(np.float64)
