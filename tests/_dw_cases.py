"""Named edge cases, the float64 reference, bounds and a mirror of the launch geometry for the depthwise 3x3 conv kernels: plain NumPy.

The entry points are ssdseg_dwconv_parts, ssdseg_dwconv_fwd, ssdseg_dwconv_bwd and ssdseg_dwconv_bwd_bn (csrc/dwconv.hip with
csrc/dwconv_march.h and csrc/dwconv_lds.h).  tests/test_cpu_dw_cases.py vets the reference, the cases and the mirror on the CPU;
tests/test_gpu_dw_edges.py runs the kernels on the same cases.  Every builder seeds its own generator from its arguments, so the
same call gives the same arrays in both files.

The lattice family.  Every input is a small multiple of a power of two, so that every product and every sum of the conv, of both
views and of all reductions is a float32 number whatever the order and whether or not a multiply-add is fused: the float64
reference IS the float32 result and the bound is 0.  `fine`: x, g, yraw, the shifts, k1, k0 and mean are multiples of 1/4, weights
of 1/8; `coarse` / `coarse1` (more than a few hundred pixels per channel): integers and weights that are multiples of 1/2; `sparse` (the
grid-stride shapes, > 10^5 pixels per channel): coarse, one value in eight non-zero, no shifts.  Scales and invstd are signed powers
of two of magnitude >= 1 (invstd: 1/2, 1, 2).  `budget` gives, in units of each result's lattice, the sum of the absolute terms of every
reduction; below 2^24 no partial sum in any order leaves the integers float32 holds exactly.  The (scale, shift) pairs put many
pre-activations exactly on 0 and exactly on 6 in both views: nothing is nudged.

The normal family.  N(0, 2) data off the lattice, pre-activations kept out of a 1e-4 band around 0 and 6, derived bounds
(U = 2^-24, gamma(L) = L U / (1 - L U)); the derivations stand in the docstring of tests/test_gpu_dw_edges.py.
"""
import functools

import numpy as np

from oracle import np_ops as O

F32 = np.float32
U = 2.0 ** -24
EXACT = 2 ** 24
ACTS = (O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6, O.ACT_ZERO)
ACT_NAMES = {O.ACT_NONE: "none", O.ACT_RELU: "relu", O.ACT_RELU6: "relu6", O.ACT_ZERO: "zero"}
MARCH_ENV = ("SSDSEG_MARCH_WAVES", "SSDSEG_MARCH_CB", "SSDSEG_MARCH_MAXT")       # read once per process: must be unset
DW_VARS = ("SSDSEG_DW_FWD", "SSDSEG_DW_BWD", "SSDSEG_DW_FWD_DEPTH", "SSDSEG_DW_ATROUS")
# the switch settings the GPU file runs every case under (all read per call)
SETTINGS = {
    "default": {},
    "march": {"SSDSEG_DW_BWD": "march"},
    "lds": {"SSDSEG_DW_FWD": "lds", "SSDSEG_DW_BWD": "lds"},
    "reg": {"SSDSEG_DW_FWD": "lds", "SSDSEG_DW_BWD": "reg"},
    "gather": {"SSDSEG_DW_ATROUS": "gather"},
    "depth1": {"SSDSEG_DW_FWD_DEPTH": "1"},
}


def gamma(length):
    return length * U / (1.0 - length * U)


def seeded(*key):
    return np.random.default_rng([1993, 3303] + [int(k) for k in key])


# =============================================================================================== mirror of the launch geometry
TW = 4                # outputs per strip of the register-window and gather kernels
MAX_BLOCKS = 1024
MTW = 4               # columns per thread of the stride-1 marches
MARCH_MIN_WAVES = 4096
LCV, LTW = 8, 16      # LDS tiles: float4 channel vectors per block, output tile width


def cdiv(a, b):
    return -(-a // b)


def same_pad(size, stride, dilation):
    """-> (out, pad before) of a 3-tap SAME conv"""
    out = cdiv(size, stride)
    total = max((out - 1) * stride + 2 * dilation + 1 - size, 0)
    return out, total // 2


def dw_geom(n, h, w, c, s, d):
    ho, pt = same_pad(h, s, d)
    wo, pl = same_pad(w, s, d)
    wtiles = cdiv(wo, TW)
    return dict(n=n, h=h, w=w, c=c, s=s, d=d, ho=ho, wo=wo, pt=pt, pl=pl, cv=c // 4, wtiles=wtiles, ntiles=n * ho * wtiles)


def march_fits(n, h, w, c):
    return n * h * w * c < (1 << 30)


def march_split(c, wstrips):
    """-> (channels per block, strips per block, channel chunks)"""
    if c > 64 and c % 64 == 0:
        cb, cchunks = 64, c // 64
    else:
        cchunks = cdiv(c, 256)
        cb = cdiv(c, cchunks)
    maxspb = min(max(256 // cb, 1), wstrips)
    best, bestwaste = 1, None
    for sp in range(maxspb, 0, -1):
        waste = cdiv(wstrips, sp) * sp - wstrips
        if bestwaste is None or (waste < bestwaste and sp * 2 > maxspb):
            best, bestwaste = sp, waste
    return cb, best, cchunks


def march_geometry(n, rows, cols, c, strip, min_waves=MARCH_MIN_WAVES, dil=1):
    """the marching kernels over `rows` x `cols` pixels per image in strips of `strip` columns.  `rows` / `chunks` / `last`: rows per
    chunk, chunks and the rows of the last chunk (of the largest sub-grid when dilated); `halvings`: how often the chunk was halved;
    `grid_x`: partial rows (blocks along x), of which the first `sblocks` have work; `row_trips`: rows one thread walks"""
    n, rows, cols = n * dil * dil, cdiv(rows, dil), cdiv(cols, dil)
    wstrips = cdiv(cols, strip)
    cb, spb, cchunks = march_split(c, wstrips)
    sgroups = cdiv(wstrips, spb)
    threads = cdiv(cb * spb, 64) * 64
    per_chunkrow = n * sgroups * cchunks * (threads // 64)
    chunk, halvings = rows, 0
    while chunk > 8 and per_chunkrow * cdiv(rows, chunk) < min_waves:
        chunk, halvings = (chunk + 1) // 2, halvings + 1
    chunks = cdiv(rows, chunk)
    sblocks = n * chunks * sgroups
    return dict(rows=chunk, chunks=chunks, last=rows - (chunks - 1) * chunk, halvings=halvings, wstrips=wstrips, cb=cb, spb=spb,
                sgroups=sgroups, cchunks=cchunks, threads=threads, sblocks=sblocks, grid_x=(sblocks + 7) & ~7,
                waves=per_chunkrow * chunks, wasted=sgroups * spb - wstrips, dil=dil, row_trips=chunk, strip=strip)


def reg_launch(g):
    """register-window and gather kernels: `live` blocks find a tile, `trips` grid-stride trips of the busiest thread"""
    bx = min(g["cv"], 256)
    by = max(min(512 // bx, 64), 1)
    gx = (max(min(cdiv(g["ntiles"], by), MAX_BLOCKS), 1) + 7) & ~7
    live = min(gx, cdiv(g["ntiles"], by))
    return dict(bx=bx, by=by, grid_x=gx, grid_y=cdiv(g["cv"], bx), live=live, trips=cdiv(g["ntiles"], gx * by))


def lds_launch(g):
    th = 8 if g["s"] == 1 else 4
    tiles = g["n"] * cdiv(g["ho"], th) * cdiv(g["wo"], LTW)
    cgroups = cdiv(g["c"], LCV * 4)
    gx = min(tiles, 1024)
    spread = gx * cgroups > 4096
    if spread:
        gx = max(4096 // cgroups, 64)
    gx = (max(min(gx, tiles), 1) + 7) & ~7
    live = min(gx, tiles)
    return dict(tiles=tiles, cgroups=cgroups, grid_x=gx, live=live, spread=spread, trips=cdiv(tiles, gx))


def _pick(env, name, values):
    return values.index(env[name]) + 1 if env.get(name) in values else 0


def fwd_family(n, h, w, c, d, env):
    lds = _pick(env, "SSDSEG_DW_FWD", ["lds"]) != 0
    atrous_ok = _pick(env, "SSDSEG_DW_ATROUS", ["gather"]) == 0
    if not lds and (d == 1 or atrous_ok) and march_fits(n, h, w, c):
        return "march"
    return "lds" if d == 1 else "gather"


def _tf(flag):
    return "true" if flag else "false"


def fwd_plan(family, n, h, w, c, s, d, env=None):
    """-> dict(family, kernel (the symbol's stem), symbol (the instantiation as the timing registry names it), rows (partial rows
    the launch writes), live (rows of blocks with work), geometry ...)"""
    g = dw_geom(n, h, w, c, s, d)
    if family == "lds":
        l = lds_launch(g)
        return dict(family=family, kernel="dw_fwd_lds_kernel", symbol=f"(dw_fwd_lds_kernel<{s}>)", rows=l["grid_x"], live=l["live"], geom=g,
                    launch=l)
    if family == "gather":
        l = reg_launch(g)
        return dict(family=family, kernel="dw_fwd_kernel", symbol="(dw_fwd_kernel<1, 0>)", rows=l["grid_x"], live=l["live"], geom=g, launch=l)
    l = march_geometry(n, g["ho"], g["wo"], c, 4 if s == 1 else 2, MARCH_MIN_WAVES, d)
    depth2 = s == 1 and d == 1 and not (env or {}).get("SSDSEG_DW_FWD_DEPTH", "").startswith("1")
    pt, pl = int(s == 1 or g["pt"] != 0), int(s == 1 or g["pl"] != 0)      # <S, PT, PL, DIL[, D2]>: stride 1 is always <1, 1, 1, ...>
    symbol = f"(dw_fwd_march_kernel<{s}, {pt}, {pl}, {_tf(d > 1)}{', true' if depth2 else ''}>)"
    return dict(family=family, kernel="dw_fwd_march_kernel", symbol=symbol, rows=l["grid_x"], live=l["sblocks"], geom=g, launch=l, depth2=depth2)


def fwd_plan_env(n, h, w, c, s, d, env):
    return fwd_plan(fwd_family(n, h, w, c, d, env), n, h, w, c, s, d, env)


def dw_fwd_table_rows(n, h, w, c, s, d):
    """ssdseg_dwconv_parts: the larger row count of the two forward kernels that can take the layer"""
    rows = 0
    for f in ("march", "lds" if d == 1 else "gather"):
        if f == "march" and not march_fits(n, h, w, c):
            continue
        rows = max(rows, fwd_plan(f, n, h, w, c, s, d)["rows"])
    return rows


def bwd_plan(n, h, w, c, s, d, env, has_dx=True, accumulate=False, has_bn=False):
    g = dw_geom(n, h, w, c, s, d)
    choice = _pick(env, "SSDSEG_DW_BWD", ["march", "lds", "reg"])
    march = choice in (0, 1) and march_fits(n, h, w, c)
    atrous_march = d > 1 and _pick(env, "SSDSEG_DW_ATROUS", ["gather"]) == 0 and g["pt"] == d and g["pl"] == d and g["ho"] == h and g["wo"] == w
    p = dict(geom=g, fuse=False)
    if march and s == 1 and (d == 1 or atrous_march):
        l = march_geometry(n, h, w, c, MTW, MARCH_MIN_WAVES, d)
        p.update(family="march", kernel="dw_bwd_march_kernel", launch=l, rows=l["grid_x"], live=l["sblocks"],
                 fuse=has_bn and d == 1 and has_dx, wfull=w % MTW == 0 and d == 1)
        p["symbol"] = f"(dw_bwd_march_kernel<{_tf(p['fuse'])}, {_tf(p['wfull'])}, {_tf(accumulate)}, {_tf(d > 1)}>)"
    elif march and s == 2 and d == 1:
        l = march_geometry(n, g["ho"], g["wo"], c, 2, MARCH_MIN_WAVES, 1)
        p.update(family="march2", kernel="dw_bwd_march2_kernel", launch=l, rows=l["grid_x"], live=l["sblocks"], fuse=has_bn and has_dx)
        p["symbol"] = f"(dw_bwd_march2_kernel<{_tf(p['fuse'])}, {int(g['pt'] != 0)}, {int(g['pl'] != 0)}, {_tf(accumulate and has_dx)}>)"
    elif d == 1 and s == 1 and (choice == 2 or (choice != 3 and c <= 160)):
        l = lds_launch(g)
        p.update(family="lds", kernel="dw_bwd_lds_kernel", symbol="(dw_bwd_lds_kernel<1, 1, 1>)", launch=l, rows=l["grid_x"], live=l["live"])
    else:
        l = reg_launch(g)
        dense = d == 1          # <S, dense taps, PT, PL>: the gather form takes its pads at run time
        p.update(family="reg" if dense else "gather", kernel="dw_bwd_kernel", launch=l, rows=l["grid_x"], live=l["live"])
        p["symbol"] = f"(dw_bwd_kernel<{s}, {int(dense)}, {int(dense and (s == 1 or g['pt'] != 0))}, {int(dense and (s == 1 or g['pl'] != 0))}>)"
    return p


def chain_length(plan, what):
    """float32 additions on the longest path into one partial row of `what` ("stats" | "dW" | "bn"): the trips of one thread times
    the additions of a trip (outputs per strip; the stride-2 backward march finalises 2 x 4 input pixels per step), then the fold
    over the block's strips"""
    l, s = plan["launch"], plan["geom"]["s"]
    per = 4 if s == 1 else 2
    if plan["family"] in ("march", "march2"):
        if what == "bn":
            per = 4 if plan["family"] == "march" else 8
        return l["row_trips"] * per + l["spb"]
    if plan["family"] == "lds":
        return l["trips"] * per + 32
    return l["trips"] * 4 + l["by"]


def unfused_chain(n, h, w, c):
    """the same for ssdseg_bn_bwd_reduce, which the families without a fused kernel run over (dx, x)"""
    import _bn_cases as BC
    m = n * h * w
    l = BC.row_launch(m, c)
    return cdiv(m, l["gx"] * l["by"]) + l["by"]


# ============================================================================================================ the cases
# name: (n, h, w, c, stride, dilation, lattice mode, forms: "all" | "large")
CASES = {}


def _case(name, shape, mode="fine", forms="all"):
    assert name not in CASES
    CASES[name] = tuple(shape) + (mode, forms)


# row chunks of the marches: stride 1 (backward over input rows = forward over output rows), two 2-strip blocks per image
for _h in (1, 2, 3, 8, 9, 13, 17, 43):
    _case(f"rows{_h}", (2, _h, 6, 8, 1, 1), "fine" if _h < 17 else "coarse")
# stride 2: the forward and the backward march over output rows
for _h, _ho in ((1, 1), (3, 2), (5, 3), (16, 8), (17, 9), (26, 13), (33, 17), (85, 43)):
    _case(f"rows{_ho}-s2", (2, _h, 7, 8, 2, 1), "fine" if _ho < 13 else "coarse")
# the halving stops midway: 2048 images of one 4-channel strip, 18 rows -> two chunks of 9 at 4096 waves
_case("halved-once", (2048, 18, 1, 4, 1, 1), "coarse")
_case("halved-once-s2", (2048, 35, 1, 4, 2, 1), "coarse")
# no halving: one chunk of 11 rows at >= 4096 waves (the form the 480 x 640 workload runs)
_case("one-chunk", (4096, 11, 5, 4, 1, 1), "sparse")
_case("one-chunk-s2", (4096, 21, 3, 4, 2, 1), "sparse")
_case("one-chunk-wide", (2, 11, 344, 1284, 1, 1), "coarse1", "large")
_case("one-chunk-wide-s2", (2, 17, 344, 1284, 2, 1), "coarse1", "large")
# columns
for _w in (1, 2, 3, 4, 5, 7, 8, 9):
    _case(f"cols{_w}", (2, 5, _w, 8, 1, 1))
_case("strips-wasted", (2, 5, 20, 64, 1, 1))          # 5 strips in two groups of 3: one wasted slot, sgroups = 2
_case("strips-wasted-s2", (2, 5, 20, 64, 2, 1))       # 10 output columns = 5 two-column strips
for _h, _w in ((5, 1), (5, 2), (6, 1), (6, 2), (5, 5), (5, 6), (6, 5), (6, 6)):       # the four pad pairs at wo = 1 and wo = 3
    _case(f"pads-{_h}x{_w}-s2", (2, _h, _w, 8, 2, 1))
# channels
for _c in (4, 60, 128, 144, 260, 1284):
    _case(f"chan{_c}", (2, 5, 6, _c, 1, 1))
    _case(f"chan{_c}-s2", (2, 5, 6, _c, 2, 1))
# dilation
_case("dil2-5x7", (2, 5, 7, 8, 1, 2))
_case("dil2-h19", (1, 19, 6, 8, 1, 2))
_case("dil6-13x13", (1, 13, 13, 8, 1, 6))
_case("dil12-4x5", (1, 4, 5, 8, 1, 12))
_case("dil3-7x5", (2, 7, 5, 8, 1, 3))
# grid-stride second trips of the other families
_case("trips-reg", (1, 520, 512, 4, 1, 1), "sparse")
_case("trips-gather", (1, 520, 512, 4, 1, 2), "sparse")
_case("trips-lds", (1, 264, 512, 4, 1, 1), "sparse")
_case("trips-lds-spread", (3, 3, 4440, 132, 1, 1), "sparse", "large")

# the one setting of the cases that exist for one family's sake; the three of 5 M elements and more also run a reduced set of forms
ONE_SETTING = {"one-chunk-wide": ("default",), "one-chunk-wide-s2": ("default",), "trips-reg": ("reg",), "trips-gather": ("gather",),
               "trips-lds": ("lds",), "trips-lds-spread": ("lds",)}


def shape_of(name):
    return CASES[name][:6]


def settings_of(name):
    """the switch settings a case runs under"""
    n, h, w, c, s, d, mode, forms = CASES[name]
    if name in ONE_SETTING:
        return ONE_SETTING[name]
    if d > 1:
        return ("default", "gather")
    return ("default", "lds", "reg", "depth1") if s == 1 else ("default", "lds")


# ------------------------------------------------------------------------------------------------------------ the forms
# forward: (input view, stats); backward: (input view, gradient view, dx, accumulate); fused: (input view, gradient view, accumulate).
# A view is "plain" | "identity" or the activation code of an affine / BatchNorm-backward view.
FWD_FORMS = [("plain", True), ("plain", False)] + [(a, a != O.ACT_RELU) for a in ACTS] + [(O.ACT_RELU6, False)]
BWD_FORMS = [("plain", "identity", True, 0), ("plain", O.ACT_RELU6, True, 1)] + \
            [(a, O.ACT_RELU6, True, i % 2) for i, a in enumerate(ACTS)] + \
            [(O.ACT_RELU6, a, True, (i + 1) % 2) for i, a in enumerate(ACTS) if a != O.ACT_RELU6] + \
            [(O.ACT_RELU6, "identity", True, 1), (O.ACT_RELU6, O.ACT_RELU6, False, 0), (O.ACT_RELU6, O.ACT_RELU6, False, 1),
             (O.ACT_RELU, "identity", False, 0)]
BN_FORMS = [(O.ACT_RELU6, O.ACT_RELU6, 0), (O.ACT_RELU6, O.ACT_RELU6, 1), (O.ACT_RELU, "identity", 1), (O.ACT_NONE, O.ACT_RELU, 0),
            (O.ACT_ZERO, O.ACT_RELU6, 1)]
LARGE_FWD_FORMS = [(O.ACT_RELU6, True)]
LARGE_BWD_FORMS = [(O.ACT_RELU6, O.ACT_RELU6, True, 0)]


def forms_of(name):
    if CASES[name][7] == "large":
        return LARGE_FWD_FORMS, LARGE_BWD_FORMS, []
    return FWD_FORMS, BWD_FORMS, BN_FORMS


def form_name(form):
    return "+".join(ACT_NAMES.get(f, str(f)) if not isinstance(f, (bool, str)) else str(f) for f in form)


# ---------------------------------------------------------------------------------------------------- lattice inputs
# (scale, shift) per channel, in turn: pre-activations on both thresholds (x = 0, +-1, +-1.5, 2 ...), both signs of the scale
PARAMS = [(1, 0), (2, 2), (-1, 1), (1, 4), (2, -1), (-2, 2), (1, -2), (4, 6)]
LATTICE = {   # mode: (denominator of x / g / yraw / shifts / k / mean, denominator of the weights, largest numerator of x, of w)
    "fine": (4, 8, 8, 3),
    "coarse": (1, 2, 2, 2),
    "coarse1": (1, 2, 2, 1),      # (the 10^7-element shapes: weights 0, +-1/2, for the sum of squares)
    "sparse": (1, 2, 3, 1),
}


class Case:
    pass


@functools.lru_cache(maxsize=2)
def lattice_case(name):
    n, h, w, c, s, d, mode, _ = CASES[name]
    xd, wd, xmax, wmax = LATTICE[mode]
    rng = seeded(*[ord(ch) for ch in name])
    ho, wo = cdiv(h, s), cdiv(w, s)
    k = Case()
    k.name, k.shape, k.mode, k.xd, k.wd = name, (n, h, w, c, s, d), mode, xd, wd
    k.ho, k.wo = ho, wo

    def grid(shape, top, den):
        return (rng.integers(-top, top + 1, shape) / den).astype(F32)

    def thin(a):
        return a * (rng.integers(0, 8, a.shape) == 0) if mode == "sparse" else a

    k.x = thin(grid((n, h, w, c), xmax, xd)).astype(F32)
    k.w = grid((3, 3, c), wmax, wd)
    k.g = thin(grid((n, ho, wo, c), xmax // 2 if mode != "sparse" else 2, xd)).astype(F32)
    k.yraw = grid((n, ho, wo, c), xmax, xd)
    k.base = thin(grid((n, h, w, c), xmax // 2 if mode != "sparse" else 2, xd)).astype(F32)
    ch = np.arange(c)
    par = np.array(PARAMS, np.float64)
    noshift = mode == "sparse"
    k.scale = par[(ch + 1) % 8, 0].astype(F32)
    k.shift = (par[(ch + 1) % 8, 1] * (0 if noshift else 1)).astype(F32)
    k.gscale = par[(ch * 3 + 2) % 8, 0].astype(F32)
    k.gshift = (par[(ch * 3 + 2) % 8, 1] * (0 if noshift else 1)).astype(F32)
    k.k1 = (((ch * 5) % 3 - 1) / xd * (0 if noshift else 1)).astype(F32)
    k.k0 = (((ch * 7) % 5 - 2) / xd * (0 if noshift else 1)).astype(F32)
    k.mean = (((ch * 3) % 5 - 2) / xd).astype(F32)
    k.invstd = np.array([1.0, 0.5, 2.0] if mode == "fine" else [1.0, 0.5, 1.0], F32)[ch % 3]
    return k


def twin_case(name):
    """the lattice case with its last image made a copy of its first: the outputs of the two must be bit-identical"""
    import copy
    k = copy.copy(lattice_case(name))
    for f in ("x", "g", "yraw", "base"):
        a = getattr(k, f).copy()
        a[-1] = a[0]
        setattr(k, f, a)
    return k


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


def g_view(k, gview, dt=np.float64, nonstrict=False):
    g = k.g.astype(dt)
    if gview == "identity":
        return g
    y, s, t = k.yraw.astype(dt), k.gscale.astype(dt), k.gshift.astype(dt)
    z = s * y + t
    m = _loose_mask(z, gview) if nonstrict else O.act_mask(z, gview)
    return s * m * g + (k.k1.astype(dt) * y + k.k0.astype(dt))


def ref_fwd(k, view, dt=np.float64):
    """-> (y, per-channel sum of y, per-channel sum of y^2)"""
    n, h, w, c, s, d = k.shape
    a, _ = in_view(k, view, dt)
    y = O.dwconv_fwd(a, k.w.astype(dt), s, d)
    return y, y.sum(axis=(0, 1, 2)), (y * y).sum(axis=(0, 1, 2))


def ref_bwd(k, view, gview, accumulate, dt=np.float64, **wrong):
    """-> (dx [+ base], dW)"""
    n, h, w, c, s, d = k.shape
    a, _ = in_view(k, view, dt)
    dy = g_view(k, gview, dt, nonstrict=wrong.get("gview_nonstrict", False))
    dx, dw = O.dwconv_bwd(a, k.w.astype(dt), dy, s, d)
    if accumulate:
        dx = dx + k.base.astype(dt)
    return dx, dw


def ref_bn(k, view, gview, accumulate, dt=np.float64, **wrong):
    """the fused form -> (dx, dW, dgamma, dbeta, k1, k0): the sums run over the COMPLETED dx"""
    n, h, w, c, s, d = k.shape
    dx, dw = ref_bwd(k, view, gview, accumulate, dt, **wrong)
    _, mask = in_view(k, view, dt, nonstrict=wrong.get("view_nonstrict", False))
    over = dx - k.base.astype(dt) if (accumulate and wrong.get("sums_before_accumulate")) else dx
    mg = over * mask
    xhat = (k.x.astype(dt) - k.mean.astype(dt)) * k.invstd.astype(dt)
    dbeta, dgamma = mg.sum(axis=(0, 1, 2)), (mg * xhat).sum(axis=(0, 1, 2))
    cnt = float(n * h * w)
    sc, istd, mu = (v.astype(np.float64) for v in (k.scale, k.invstd, k.mean))
    dg64, db64 = dgamma.astype(np.float64), dbeta.astype(np.float64)
    k1 = -sc * dg64 * istd / cnt
    k0 = sc * (dg64 * istd * mu - db64) / cnt
    kbound = (U * np.abs(k1) + 2.0 ** -50 * np.abs(sc * dg64 * istd) / cnt,
              U * np.abs(k0) + 2.0 ** -50 * np.abs(sc) * (np.abs(dg64 * istd * mu) + np.abs(db64)) / cnt)
    return dx, dw, dgamma, dbeta, k1, k0, kbound


def budget(k, views=None):
    """sum of the absolute terms of every reduction, in units of the result's lattice; < 2^24 = every partial sum in any order, fused
    or not, is exact.  The forward's statistics over the actual y of each input view the case runs (their terms are |y| and y^2);
    the backward's over the worst view of each side (no clamp, every mask 1), the accumulation base included"""
    n, h, w, c, s, d = k.shape
    xd, wd = float(k.xd), float(k.wd)
    if views is None:
        views = sorted({f[0] for f in forms_of(k.name)[0]}, key=str)
    x = np.abs(k.x.astype(np.float64))
    a = np.maximum(x, np.abs(k.x.astype(np.float64) * k.scale) + np.abs(k.shift.astype(np.float64)))
    wa = np.abs(k.w.astype(np.float64))
    y = k.yraw.astype(np.float64)
    dy = np.abs(k.gscale * k.g.astype(np.float64)) + np.abs(k.k1 * y) + np.abs(k.k0.astype(np.float64))
    yabs = O.dwconv_fwd(a, wa, s, d)
    dxabs, dwabs = O.dwconv_bwd(a, wa, dy, s, d)
    dxabs = dxabs + np.abs(k.base)
    xhat = (x + np.abs(k.mean)) * k.invstd
    ua, uw, udy, uhat = 1 / xd, 1 / wd, 1 / (xd * xd), 1 / (2 * xd)
    ssum = ssq = 0.0
    for view in views:
        yv = ref_fwd(k, view)[0]
        ssum = max(ssum, np.abs(yv).sum(axis=(0, 1, 2)).max())
        ssq = max(ssq, (yv * yv).sum(axis=(0, 1, 2)).max())
    return {
        "y": yabs.max() / (ua * uw),
        "y*y": (yabs * yabs).max() / (ua * uw) ** 2,
        "sum": ssum / (ua * uw),
        "sumsq": ssq / (ua * uw) ** 2,
        "dy": dy.max() / udy,
        "dx": dxabs.max() / (udy * uw),
        "dW": dwabs.max() / (ua * udy),
        "dbeta": dxabs.sum(axis=(0, 1, 2)).max() / (udy * uw),
        "dgamma": (dxabs * xhat).sum(axis=(0, 1, 2)).max() / (udy * uw * uhat),
    }


# ------------------------------------------------------------------------------------------------------ the normal family
NORMAL_CASES = ["rows9", "rows17-s2", "cols7", "strips-wasted", "chan260", "chan144-s2", "dil2-h19", "dil3-7x5", "pads-6x5-s2"]
BAND = 1e-4


def _off_thresholds(v, s, t):
    """values whose pre-activation s v + t lies within BAND of 0 or 6 moved by 0.05 -> (values, share moved)"""
    z = v.astype(np.float64) * s + t
    near = (np.abs(z) < BAND) | (np.abs(z - 6) < BAND)
    return np.where(near, v + F32(0.05), v).astype(F32), float(near.mean())


@functools.lru_cache(maxsize=2)
def normal_case(name):
    n, h, w, c, s, d, _, _ = CASES[name]
    rng = seeded(7, *[ord(ch) for ch in name])
    ho, wo = cdiv(h, s), cdiv(w, s)
    k = Case()
    k.name, k.shape, k.mode, k.ho, k.wo = name, (n, h, w, c, s, d), "normal", ho, wo
    k.scale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c, p=[0.25, 0.75])).astype(F32)
    k.shift = rng.uniform(-1, 3, c).astype(F32)
    k.gscale = rng.uniform(0.5, 1.5, c).astype(F32)
    k.gshift = rng.uniform(-1, 3, c).astype(F32)
    k.x, k.nudged_x = _off_thresholds(rng.normal(0, 2, (n, h, w, c)).astype(F32), k.scale, k.shift)
    k.yraw, k.nudged_y = _off_thresholds(rng.normal(0, 2, (n, ho, wo, c)).astype(F32), k.gscale, k.gshift)
    k.w = rng.normal(0, 0.3, (3, 3, c)).astype(F32)
    k.g = rng.normal(0, 2, (n, ho, wo, c)).astype(F32)
    k.base = rng.normal(0, 2, (n, h, w, c)).astype(F32)
    k.k1 = rng.normal(0, 0.1, c).astype(F32)
    k.k0 = rng.normal(0, 0.1, c).astype(F32)
    k.mean = k.x.mean(axis=(0, 1, 2), dtype=np.float64).astype(F32)
    k.invstd = (1.0 / np.sqrt(k.x.var(axis=(0, 1, 2), dtype=np.float64) + 1e-3)).astype(F32)
    return k


def normal_bounds(k, view, gview, accumulate, fplan, bplan):
    """per-element and per-channel bounds of one form of a normal case (derivations: tests/test_gpu_dw_edges.py)"""
    n, h, w, c, s, d = k.shape
    x = k.x.astype(np.float64)
    za = np.abs(x) if view == "plain" else np.abs(x * k.scale) + np.abs(k.shift.astype(np.float64))      # |s x| + |t| >= |z|, |a|
    a, mask = in_view(k, view)
    wa = np.abs(k.w.astype(np.float64))
    # forward: the view's one rounding (U |z|) on every tap, nine multiply-adds
    yabs = O.dwconv_fwd(za, wa, s, d)
    y_b = (gamma(10) + U) * yabs
    y, _, _ = ref_fwd(k, view)
    lf = chain_length(fplan, "stats")
    sum_b = gamma(lf + 1) * np.abs(y).sum(axis=(0, 1, 2)) + y_b.sum(axis=(0, 1, 2))
    sq_b = gamma(lf + 2) * (y * y).sum(axis=(0, 1, 2)) + (2 * np.abs(y) * y_b + y_b * y_b).sum(axis=(0, 1, 2))
    # backward: dy carries two roundings of its absolute terms
    g, yr = k.g.astype(np.float64), k.yraw.astype(np.float64)
    dyabs = np.abs(g) if gview == "identity" else np.abs(k.gscale * g) + np.abs(k.k1 * yr) + np.abs(k.k0.astype(np.float64))
    dxabs, dwabs = O.dwconv_bwd(za, wa, dyabs, s, d)
    dx_b = (gamma(10) + 2 * U) * dxabs
    dx, dw = ref_bwd(k, view, gview, accumulate)
    if accumulate:
        dx_b = dx_b + U * (np.abs(dx) + dx_b)
    lw = chain_length(bplan, "dW")
    dw_b = (gamma(lw + 2) + 3 * U) * dwabs + U * np.abs(dw)
    # fused sums: over the completed dx, xhat = (x - mean) * invstd with two roundings
    xhat = np.abs((x - k.mean) * k.invstd)
    lb = chain_length(bplan, "bn") if bplan["fuse"] else unfused_chain(n, h, w, c)
    mdx = np.abs(dx * mask)
    dbeta_b = gamma(lb + 1) * mdx.sum(axis=(0, 1, 2)) + (dx_b * mask).sum(axis=(0, 1, 2))
    dgamma_b = (gamma(lb + 2) + 2 * U) * (mdx * xhat).sum(axis=(0, 1, 2)) + (dx_b * mask * xhat).sum(axis=(0, 1, 2))
    return dict(y=y_b, sum=sum_b, sumsq=sq_b, dx=dx_b, dW=dw_b, dbeta=dbeta_b + U * np.abs((dx * mask).sum(axis=(0, 1, 2))),
                dgamma=dgamma_b + U * np.abs((dx * mask * (x - k.mean) * k.invstd).sum(axis=(0, 1, 2))))


# ------------------------------------------------------------------------------ structural errors, shown on the reference
def conv_fwd_pads(a, w, s, d, pt, pl):
    """the forward with explicit leading pads (the right ones: same_pad): what a kernel with a wrong pad computes"""
    n, h, wd, c = a.shape
    ho, wo = cdiv(h, s), cdiv(wd, s)
    need_h, need_w = (ho - 1) * s + 2 * d + 1, (wo - 1) * s + 2 * d + 1
    xp = np.zeros((n, pt + max(need_h, h) + 2 * d + 2, pl + max(need_w, wd) + 2 * d + 2, c), a.dtype)
    xp[:, pt:pt + h, pl:pl + wd] = a
    y = np.zeros((n, ho, wo, c), a.dtype)
    for kh in range(3):
        for kw in range(3):
            y += xp[:, kh * d: kh * d + (ho - 1) * s + 1: s, kw * d: kw * d + (wo - 1) * s + 1: s] * w[kh, kw]
    return y


def row_terms(k, view, gview):
    """what each output row contributes -> (the sum of y over the row, (ho, c); the dW terms of the row's dy, (ho, 3, 3, c))"""
    n, h, w, c, s, d = k.shape
    a, _ = in_view(k, view)
    dy = g_view(k, gview)
    y = O.dwconv_fwd(a, k.w.astype(np.float64), s, d)
    rows = []
    for r in range(k.ho):
        only = np.zeros_like(dy)
        only[:, r] = dy[:, r]
        rows.append(O.dwconv_bwd(a, k.w.astype(np.float64), only, s, d)[1])
    return y.sum(axis=(0, 2)), np.array(rows)


# ------------------------------------------------------------------------------------- a mixed batch of deferred column sums
# Four ssdseg_dwconv_bwd calls (stride 1, dilation 1, default switches) whose weight-gradient slab tables take every route of the
# column-sum dispatch (csrc/colsum.hip): few rows; exactly at the 32-row switch; exactly at the 256-row switch; the wide route.
# (n, h, w, c): (partial rows of the slab table, channels per block of its column sum)
COLSUM_MIX = {(1, 8, 12, 8): (8, 32), (2, 128, 128, 8): (32, 8), (2, 256, 256, 16): (256, 2), (1, 8, 8, 512): (8, 32)}
COLSUM_WIDE = 4096


def colsum_rc(nparts, length):
    """columns per block of a column sum: mirror of colsum_rc in csrc/colsum.hip (without its A/B environment switch)"""
    import _bn_cases as BC
    return 32 if length >= COLSUM_WIDE else BC.reduce_rc(nparts, length)


def colsum_mix_case(shape):
    """x, w, two different g on the integer lattice {-3 .. 3} -> (x, w, g, g_other): with an identity view and an identity gradient
    view every partial and every column sum of dW is an integer of at most 9 n h w < 2^24 (|x g| <= 9 per pixel), exact in float32
    in any order"""
    n, h, w, c = shape
    assert 9 * n * h * w < EXACT
    rng = seeded(77, *shape)
    x, g, other = (rng.integers(-3, 4, (n, h, w, c)).astype(F32) for _ in range(3))
    return x, rng.integers(-3, 4, (3, 3, c)).astype(F32), g, other
