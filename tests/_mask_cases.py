"""Named edge cases, float64 references and derived error bounds for the bilinear resize and the mask head: plain NumPy.

The entry points are ssdseg_bilinear_fwd / _fwd_padded / _bwd (csrc/resize.hip: a general kernel and an x4 kernel each) and
ssdseg_mask_head_fwd / _bwd / _fwd_dice / _bwd_dice / _fwd_bootstrap / _bwd_bootstrap (csrc/mask_head.hip: the fused up-sampling,
softmax and loss forward; the gather, x4 tile and x8 split-tile backward kernels).  tests/test_cpu_mask_cases.py vets the
references, the cases and the bounds on the CPU; tests/test_gpu_mask_edges.py runs the kernels on the same cases.  Every builder
seeds its own generator from its arguments, so the same call gives the same arrays in both files.

Inputs live on a lattice: logits, bilinear inputs and gradients are multiples of 1/4 of bounded magnitude.  With a power-of-two
factor up to 16 every blend fraction is k/32, so every difference, product and sum of lerp_blend4 (quanta 1/4, 1/128, 1/4096;
magnitudes below 2^24 quanta) is a float32 number: the float64 reference of the up-sampling IS the float32 result, bound 0, and the
logits the softmax sees carry no error (zerr = 0 in softmax_bound).  The same holds for the backward: every term wy wx g is a
multiple of 2^-12 and every partial sum stays below 2^24 of them, whatever the order.

U = 2^-24, ULP = 2^-23; gamma(L) as in tests/_tail_cases.py, whose softmax_bound, logits_prob_error and gamma are used as they stand.
"""
import numpy as np

import _tail_cases as TC
from oracle import np_ops as O

F32 = np.float32
U, ULP, TINY = TC.U, TC.ULP, TC.TINY
gamma, seeded, w64 = TC.gamma, TC.seeded, TC.w64
SECOND_ORDER = TC.SECOND_ORDER
CW, CW_ZERO = TC.CW, TC.CW_ZERO
CW_NONE, CW_ONE = (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)
LO = float(TC.LO32)                      # the device's clip interval: float32(1e-7) and float32(1) - float32(1e-7) = 1 - 2^-23
HI = float(TC.HI32)
QUANTUM = 0.25                           # the lattice
DECIDE = 10.0                            # an entry within DECIDE x its softmax bound of LO is undecidable
SEEDS = 4                                # the case builder takes the first of this many seeds without an undecidable entry


def pow2(f):
    return f & (f - 1) == 0


def lattice(rng, shape, mag):
    """multiples of 1/4 in [-mag, mag] as float32"""
    k = int(mag / QUANTUM)
    return (rng.integers(-k, k + 1, shape) * QUANTUM).astype(F32)


# ------------------------------------------------------------------------------------------------- launch mirrors
TL4, TL8, PARTS8 = 16, 8, 4
EW_CAP = 8192                            # ew_blocks: at most this many 256-thread blocks


def partial_blocks(npix, cap=256):
    """mirror of partial_blocks in csrc/mask_head.hip: blocks per image (eight pixels per thread) and the trips of a thread"""
    nblk = max(1, min((npix + 2047) // 2048, cap))
    return dict(nblk=nblk, trips=-(-npix // (nblk * 256)))


def ew_blocks(total):
    """mirror of ew_blocks in csrc/common.h: blocks, and the trips of a thread of the grid-stride loop"""
    b = max(1, min((total + 255) // 256, EW_CAP))
    return dict(blocks=b, trips=-(-total // (b * 256)))


def mask_bwd_dispatch(n, h, w, fy, fx, gather=False):
    """mirror of mask_head_bwd_launch: the kernel's name in the timing registry and its block count"""
    if not gather and fy == 4 and fx == 4:
        return "(mask_head_bwd_tile_kernel<F, TL>)", n * -(-h // TL4) * -(-w // TL4)
    if not gather and fy == 8 and fx == 8:
        return "(mask_head_bwd_tile_split_kernel<F, TL, PARTS>)", n * -(-h // TL8) * -(-w // TL8)
    return "mask_head_bwd_kernel", ew_blocks(n * h * w)["blocks"]


def bilinear_dispatch(n, h, w, c, fy, fx, backward=False, accumulate=0, pitched=False, gather=False):
    """mirror of ssdseg_bilinear_fwd / _bwd: {kernel: launches}"""
    x4 = fy == 4 and fx == 4 and not gather
    if backward and h == 1 and w == 1:
        return TC.pixel_sum_launch(n, fy * fx, c, accumulate, pitched)["kernels"]
    if backward:
        return {"bilinear_bwd_x4_kernel" if x4 else "bilinear_bwd_kernel": 1}
    return {"bilinear_fwd_x4_kernel" if x4 else "bilinear_fwd_kernel": 1}


# ------------------------------------------------------------------------------------------------- geometry
def axis_weights(in_size, f):
    """(out, in) float64 matrix of the half-pixel bilinear weights of one axis (O._bilinear_axis as a matrix)"""
    i0, i1, fr = O._bilinear_axis(in_size, f, np.float64)
    m = np.zeros((in_size * f, in_size))
    np.add.at(m, (np.arange(in_size * f), i0), 1.0 - fr)
    np.add.at(m, (np.arange(in_size * f), i1), fr)
    return m


def axis_src_error(in_size, f):
    """|dsrc| of every output index: lerp_of forms (dst + 0.5) fl(1 / f) - 0.5 in float32 -- the reciprocal, the product and the
    difference are three roundings of at most (dst + 0.5) / f: 3 U (dst + 0.5) / f.  A power of two has an exact reciprocal, the
    product is a shift and the difference of two multiples of 1 / 2f below 2^24 of them is exact: 0.  The clamp never enlarges it."""
    if pow2(f):
        return np.zeros(in_size * f)
    return 3 * U * (np.arange(in_size * f) + 0.5) / f


def axis_weight_error(in_size, f):
    """(out, in) bound on the error of a weight: the hat function has slope 1, so a weight moves by at most |dsrc| -- also where
    floor flips, and for an input next to the support (weight 0 in the reference, up to |dsrc| on the device); 1 - f is one more
    rounding (U)."""
    ds = axis_src_error(in_size, f)
    if not ds.any():
        return np.zeros((in_size * f, in_size))
    src = np.clip((np.arange(in_size * f) + 0.5) / f - 0.5, 0, in_size - 1)
    near = np.abs(src[:, None] - np.arange(in_size)[None, :]) <= 1.0 + 1e-6
    return (ds[:, None] + U) * near


def up(x, fy, fx):
    return O.bilinear_fwd(np.asarray(x, np.float64), fy, fx)


def is_identity(m):
    return m.shape[0] == m.shape[1] and np.array_equal(m, np.eye(m.shape[0]))


def down(g, wy, wx):
    """transposed resize with the given (out, in) axis matrices: (n, ho, wo, c) -> (n, h, w, c)"""
    g = np.asarray(g, np.float64)
    if not is_identity(wy):
        g = np.einsum("oh,nopc->nhpc", wy, g, optimize=True)
    if not is_identity(wx):
        g = np.einsum("nhpc,pw->nhwc", g, wx, optimize=True)
    return g


def window_terms(h, w, fy, fx):
    """the largest number of non-zero weights an input pixel has: the length of the backward kernels' chains"""
    return int((axis_weights(h, fy) != 0).sum(0).max() * (axis_weights(w, fx) != 0).sum(0).max())


# ------------------------------------------------------------------------------------------------- bilinear
# (n, h, w, c, fy, fx)
BILINEAR_SHAPES = [(2, 1, 5, 4, 3, 2), (1, 5, 1, 8, 2, 3), (1, 3, 4, 4, 1, 1), (2, 3, 5, 12, 3, 5), (1, 4, 3, 4, 6, 1), (1, 2, 2, 4, 16, 16),
                   (1, 7, 9, 8, 4, 8), (1, 5, 7, 8, 8, 4)]
X4_SHAPES = [(1, 1, 1), (2, 1, 6), (2, 6, 1), (1, 2, 2), (1, 3, 5), (3, 7, 8), (1, 16, 17)]          # (n, h, w)
X4_CHANNELS = (4, 12, 260)               # cv = 1, 3, 65
PADDED_FACTORS = [(2, 2), (4, 4), (3, 5)]
BILINEAR_FWD_TRIP = (1, 65, 64, 8, 16, 16)
BILINEAR_BWD_TRIP = (1, 1025, 1024, 8, 1, 1)
X_MAG, G_MAG = 120.0, 4.0


def bilinear_input(n, h, w, c):
    return lattice(seeded(40, n, h, w, c), (n, h, w, c), X_MAG)


def bilinear_grad(n, ho, wo, c):
    return lattice(seeded(41, n, ho, wo, c), (n, ho, wo, c), G_MAG)


def lerp_rounding(a, b, ea, eb):
    """error bound of fl(a + (b - a) f) for any f in [0, 1]: the operands' errors pass through a convex combination (their
    maximum); the difference, the product and the sum are three roundings, of |b - a|, at most |b - a| and at most max(|a|, |b|)"""
    return np.maximum(ea, eb) + U * (2 * np.abs(b - a) + np.maximum(np.abs(a), np.abs(b)))


def bilinear_fwd_bound(a, fy, fx, mag=None, exact=False):
    """a: the activated input in float64, (n, h, w, c).  exact (lattice input, plain view, power-of-two factors): 0.  Otherwise
    per output: the corner values carry the view's rounding (ULP of mag = |s x| + |t|, as in the tail suite; the activation's clamp
    never enlarges it); lerp_blend4 is two levels of lerp_rounding; the blend is continuous and piecewise linear in the source
    coordinate, so it moves by at most |dsrc| times the steepest step between neighbouring inputs along that axis, taken over the
    image (which also covers a flip of floor): axis_src_error."""
    n, h, w, c = a.shape
    if exact:
        return np.zeros((n, h * fy, w * fx, c))
    y0, y1, _ = O._bilinear_axis(h, fy, np.float64)
    x0, x1, _ = O._bilinear_axis(w, fx, np.float64)
    e = ULP * np.asarray(mag, np.float64) if mag is not None else np.zeros_like(a)
    corner = lambda v, yy, xx: v[:, yy][:, :, xx]
    top = lerp_rounding(corner(a, y0, x0), corner(a, y0, x1), corner(e, y0, x0), corner(e, y0, x1))
    bot = lerp_rounding(corner(a, y1, x0), corner(a, y1, x1), corner(e, y1, x0), corner(e, y1, x1))
    tv = np.maximum(np.abs(corner(a, y0, x0)), np.abs(corner(a, y0, x1)))
    bv = np.maximum(np.abs(corner(a, y1, x0)), np.abs(corner(a, y1, x1)))
    out = np.maximum(top, bot) + U * (2 * (tv + bv) + np.maximum(tv, bv))
    step_y = np.abs(np.diff(a, axis=1)).max(axis=(1, 2), keepdims=True) if h > 1 else 0.0
    step_x = np.abs(np.diff(a, axis=2)).max(axis=(1, 2), keepdims=True) if w > 1 else 0.0
    out = out + axis_src_error(h, fy)[None, :, None, None] * step_y + axis_src_error(w, fx)[None, None, :, None] * step_x
    return SECOND_ORDER * out


def bilinear_bwd_terms(g, h, w, fy, fx):
    """sum over the window of |wy wx g|: what the chain's gamma multiplies, and what the lattice argument bounds"""
    return down(np.abs(np.asarray(g, np.float64)), axis_weights(h, fy), axis_weights(w, fx))


def bilinear_bwd_bound(g, h, w, fy, fx, exact=False):
    """exact (lattice gradient, power-of-two factors): 0 -- every term is a multiple of 2^-12, every partial sum below 2^24 of them
    (asserted on the CPU), so no summation order rounds.  Otherwise: each weight carries axis_weight_error, the product wy wx one
    rounding, and the chain of fused multiply-adds over the K window terms gamma(K); first order:
    sum |g| (dwy wx + wy dwx + dwy dwx) + gamma(K + 1) sum |g| wy wx."""
    if exact:
        return np.zeros((g.shape[0], h, w, g.shape[3]))
    ag = np.abs(np.asarray(g, np.float64))
    wy, wx, dy, dx = axis_weights(h, fy), axis_weights(w, fx), axis_weight_error(h, fy), axis_weight_error(w, fx)
    moved = down(ag, dy, wx) + down(ag, wy, dx) + down(ag, dy, dx)
    return SECOND_ORDER * (moved + gamma(window_terms(h, w, fy, fx) + 1) * down(ag, wy, wx))


# ------------------------------------------------------------------------------------------------- mask head: shapes
# (n, h, w, fy, fx): the smallest that reach each edge of a tile kernel, every factor pair of the gather kernel, and the capped grids
MASK_X4_SHAPES = [(1, 1, 1, 4, 4), (2, 1, 17, 4, 4), (2, 17, 1, 4, 4), (1, 16, 16, 4, 4), (1, 15, 33, 4, 4), (2, 32, 17, 4, 4)]
MASK_X8_SHAPES = [(1, 1, 1, 8, 8), (2, 1, 9, 8, 8), (2, 9, 1, 8, 8), (1, 8, 8, 8, 8), (1, 7, 17, 8, 8), (2, 16, 9, 8, 8)]
MASK_GATHER_SHAPES = [(1, 3, 5, 1, 1), (2, 3, 4, 2, 2), (1, 4, 3, 3, 5), (1, 2, 5, 4, 8), (1, 5, 2, 8, 4), (1, 2, 2, 16, 16)]
MASK_FWD_CAP = (1, 182, 182, 4, 4)       # 529,984 pixels: 256 blocks and a ninth trip
MASK_BWD_TRIP = (2, 1025, 1024, 1, 1)    # 2,099,200 threads: a second grid-stride trip of the gather backward
MASK_SMALL_SHAPES = MASK_X4_SHAPES + MASK_X8_SHAPES + MASK_GATHER_SHAPES
MASK_SHAPES = MASK_SMALL_SHAPES + [MASK_FWD_CAP, MASK_BWD_TRIP]
FAMILIES = {"moderate": 6.0, "clip": 30.0, "extreme": 120.0, "offset": 6.0, "normal": None}
LOSS_SCALES = (0.5, None, -1.0)          # None: 1 / n
WEIGHTS = (CW, CW_ZERO, CW_ONE)


def mask_settings(shape, k):
    """the class weights and the loss scale of the k-th run of a shape: with i = the shape's index + k the weights walk with i and the
    scales with i // 3, so nine consecutive i meet every pair (each of the x4, x8 and gather lists spans at least ten)"""
    i = MASK_SHAPES.index(shape) + k
    scale = LOSS_SCALES[(i // 3) % 3]
    return WEIGHTS[i % 3], (1.0 / shape[0] if scale is None else scale)


def mask_logits(shape, family, seed):
    n, h, w, fy, fx = shape
    rng = seeded(42, n, h, w, fy, fx, list(FAMILIES).index(family), seed)
    if family == "normal":
        return rng.normal(0, 2, (n, h, w, 4)).astype(F32)
    z = lattice(rng, (n, h, w, 4), FAMILIES[family])
    return z + F32(1000.0) if family == "offset" else z


def mask_labels(shape, kind="mixed", p=None):
    """(n, ho wo, 4) float32.  mixed: of every 16 pixels (in a seeded order; pixel order[0] is always void) one is void (all zero:
    6 %), two are soft (multiples of 1/8 that sum to 1), one is multi-hot (two or three ones), the rest one-hot.  dice: one-hot with
    void rows, class 3 absent from image 0, and the last image of a batch all void; given the probabilities p, the labels agree
    with them (their arg-max) in the 256-pixel groups a hash picks and are random in the others, as TC.graded_probs does it the other
    way round: the ratio I / T of a partial block is then never the image's, so no lost block is representative."""
    n, h, w, fy, fx = shape
    npix = h * fy * w * fx
    rng = seeded(43, n, h, w, fy, fx)
    y = TC.one_hot_rows(rng, (n, npix))
    for i in range(n):
        order = rng.permutation(npix)
        kind_of = np.empty(npix, np.int64)
        kind_of[order] = np.arange(npix) % 16
        y[i, kind_of == 0] = 0.0
        if kind == "mixed":
            soft = np.flatnonzero((kind_of == 1) | (kind_of == 2))
            cuts = np.sort(rng.integers(0, 9, (soft.size, 3)), axis=1)
            y[i, soft] = (np.diff(np.concatenate([np.zeros((soft.size, 1), np.int64), cuts, np.full((soft.size, 1), 8)], axis=1), axis=1) / 8).astype(F32)
            multi = np.flatnonzero(kind_of == 3)
            rows = (rng.integers(0, 2, (multi.size, 4)) > 0)
            rows[np.arange(multi.size), rng.integers(0, 4, multi.size)] = True
            rows[np.arange(multi.size), (rng.integers(0, 4, multi.size) + 1) % 4] = True
            y[i, multi] = rows.astype(F32)
    if kind == "dice" and p is not None:
        group = (np.arange(npix) // 256) % 64
        strong = ((group * 40503 >> 3) & 1).astype(bool)
        agree = np.eye(4, dtype=F32)[p.argmax(-1)]
        y = np.where(strong[None, :, None] & y.any(-1, keepdims=True), agree, y).astype(F32)
    if kind == "dice":
        cls = y[0].argmax(-1)
        y[0] = np.where(y[0].any(-1, keepdims=True), np.eye(4, dtype=F32)[np.where(cls == 3, 1, cls)], 0).astype(F32)
        if n > 1:
            y[-1] = 0.0
    return y


# ------------------------------------------------------------------------------------------------- mask head: references
def logit_error(logits, fy, fx, family):
    """absolute error of an up-sampled logit: 0 on the lattice with power-of-two factors, else bilinear_fwd_bound, the largest of a
    pixel's four classes, (n, ho, wo, 1).  ("normal" with power-of-two factors goes through TC.logits_prob_error instead.)"""
    exact = family != "normal" and pow2(fy) and pow2(fx)
    return bilinear_fwd_bound(np.asarray(logits, np.float64), fy, fx, exact=exact).max(-1, keepdims=True)


def prob_ref(logits, fy, fx, family="clip"):
    """(p, bp): float64 probabilities (n, ho wo, 4) and the absolute bound of each.  TC.softmax_bound with the logit's error; for
    the normal family with power-of-two factors TC.logits_prob_error (relative) -- its own count of the same roundings"""
    n = logits.shape[0]
    z = up(logits, fy, fx)
    p = O.softmax(z).reshape(n, -1, 4)
    if family == "normal" and pow2(fy) and pow2(fx):
        bp = SECOND_ORDER * TC.logits_prob_error(float(np.abs(logits).max())) * p + TINY
    else:
        bp = TC.softmax_bound(z, logit_error(logits, fy, fx, family)).reshape(n, -1, 4)
    return p, bp


def undecidable(y, p, bp):
    """labelled entries whose probability is within DECIDE bounds of the lower clip bound: float32 cannot be asked which side they
    are on.  (The upper bound needs no such rule, see dz_bound.)"""
    return (y != 0) & (np.abs(p - LO) <= DECIDE * bp)


def mask_case(shape, family, kind="mixed"):
    """dict(logits, y, p, bp, seed): the first of SEEDS seeds whose reference has no undecidable entry (None when there is none)"""
    fy, fx = shape[3:]
    y = mask_labels(shape, kind)
    for seed in range(SEEDS):
        logits = mask_logits(shape, family, seed)
        p, bp = prob_ref(logits, fy, fx, family)
        if kind == "dice":
            y = mask_labels(shape, kind, p)
        if not undecidable(y, p, bp).any():
            return dict(logits=logits, y=y, p=p, bp=bp, seed=seed, family=family, shape=shape)
    return None


def clip_sides(y, p):
    """share of the labelled entries below / not below the lower clip bound"""
    lab = y != 0
    below = float(((p < LO) & lab).sum()) / max(1, int(lab.sum()))
    return below, 1.0 - below


def inside64(p, lo=LO, hi=HI):
    return ((p >= lo) & (p <= hi)).astype(np.float64)


def ce_terms(y, p, weights, lo=LO, hi=HI):
    """(n, npix, 4) terms -w_c y_c log(clip p_c) with the device's float32 clip bounds as float64 numbers"""
    return -w64(weights) * y.astype(np.float64) * np.log(np.clip(p, lo, hi))


def ce_ref(y, p, weights, lo=LO, hi=HI):
    return ce_terms(y, p, weights, lo, hi).sum(axis=(1, 2))


def ce_pixel_ref(y, p, weights):
    return ce_terms(y, p, weights).sum(-1)


def ce_dp(y, p, weights, lo=LO, hi=HI, clip_rule=True):
    """dL/dp of the cross-entropy: -w y / clip(p) inside the clip interval, 0 outside (clip_rule=False: never zeroed)"""
    dp = -w64(weights) * y.astype(np.float64) / np.clip(p, lo, hi)
    return dp * inside64(p, lo, hi) if clip_rule else dp


def ce_bound(y, p, bp, weights):
    """Per term: log(clip p) moves by at most bp / max(p, lo) (the clipped logarithm is continuous with slope 1 / p inside and 0
    outside), logf is 2 ulp (4 U |log|), w y, its product with the logarithm, the three additions of a pixel's four terms and
    `loss -=` are 6 roundings; a thread adds `trips` pixels, the block tree has 8 levels; the fold is in double and its cast to
    float one rounding: gamma(trips + 8 + 7) of the sum of absolute terms."""
    la = partial_blocks(y.shape[1])
    wy = np.abs(w64(weights) * y.astype(np.float64))
    logp = np.abs(np.log(np.clip(p, LO, HI)))
    per_term = wy * (bp / np.maximum(p, LO) + 4 * U * logp)
    return SECOND_ORDER * (per_term.sum(axis=(1, 2)) + gamma(la["trips"] + 8 + 7) * (wy * logp).sum(axis=(1, 2)))


def dice_sums(y, p, squared):
    y64 = y.astype(np.float64)
    return (y64 * p).sum(1), ((y64 * y64 + p * p) if squared else (y64 + p)).sum(1)


def dice_ref(y, p, weights, squared):
    """(loss (n,), coef (n, 8) = (A_c, B_c)): mask_dice_final_kernel's closed form in float64 with the device's float32 epsilon"""
    w = w64(weights)
    inter, total = dice_sums(y, p, squared)
    den, num = total + TC.KEPS32, 2 * inter + TC.KEPS32
    return (w * (1 - num / den)).sum(-1), np.concatenate([-2 * w / den, w * num / den ** 2], axis=-1)


def dice_dp(y, p, coef, squared):
    t = 2 * p if squared else np.ones_like(p)
    return coef[:, None, :4] * y.astype(np.float64) + coef[:, None, 4:] * t


def dice_sum_errors(y, p, bp, squared):
    """absolute errors of I_c and T_c: a term carries bp (y bp in I; bp or 2 p bp in T) and its own roundings (I: the fused
    multiply-add is the chain's; T: y + p is 1, y^2 + p^2 is 2 and the addition to the sum); the chain is trips + 8 tree levels, the
    fold is in double"""
    la = partial_blocks(y.shape[1])
    y64 = y.astype(np.float64)
    inter, total = dice_sums(y, p, squared)
    chain = la["trips"] + 8
    d_inter = (y64 * bp).sum(1) + gamma(chain + 1) * inter
    d_total = ((2 * p * bp) if squared else bp).sum(1) + gamma(chain + 3) * total
    return d_inter, d_total


def dice_bound(y, p, bp, weights, squared):
    """TC.dice_bound's argument with the sums' errors above: r = (2 I + e) / (T + e) moves by (2 dI + r dT) / (T + e); the closed
    form is evaluated in double, the cast of the loss to float is one rounding"""
    w = np.abs(w64(weights))
    inter, total = dice_sums(y, p, squared)
    d_inter, d_total = dice_sum_errors(y, p, bp, squared)
    den = total + TC.KEPS32
    r = (2 * inter + TC.KEPS32) / den
    return SECOND_ORDER * ((w * (2 * d_inter + r * d_total) / den).sum(-1) + U * (w * np.abs(1 - r)).sum(-1))


def dice_coef_error(y, p, bp, weights, squared):
    """(n, 8) absolute errors of (A_c, B_c) as floats: A = -2 w / D moves by |A| dD / D, B = w N / D^2 by |B| (dN / N + 2 dD / D),
    and each is rounded to float once"""
    _, coef = dice_ref(y, p, weights, squared)
    inter, total = dice_sums(y, p, squared)
    d_inter, d_total = dice_sum_errors(y, p, bp, squared)
    den, num = total + TC.KEPS32, 2 * inter + TC.KEPS32
    rel_a = d_total / den + U
    rel_b = 2 * d_inter / num + 2 * d_total / den + U
    return np.abs(coef) * np.concatenate([rel_a, rel_b], axis=-1)


def dz_of(p, dp):
    return O.softmax_bwd(p, dp)


def dz_bound(p, bp, dp, ddp):
    """dz_c = p_c (dp_c - dot), dot = sum_k dp_k p_k, per full-resolution pixel.  With the absolute errors bp of p and ddp of dp:
    dot's four products carry |dp_k| bp_k + p_k ddp_k and a rounding each, its three additions 3 U of the absolute sum S = sum |dp_k|
    p_k; dp_c - dot is one rounding of at most |dp_c| + S; the product with p_c one more and p_c's own error.  Because dp_c - dot
    cancels as p_c -> 1 the result is absolute on the scale p_c (|dp_c| + S), not relative to dz."""
    s = (np.abs(dp) * p).sum(-1, keepdims=True)
    ddot = (np.abs(dp) * bp + p * ddp).sum(-1, keepdims=True) + 4 * U * s
    return p * (ddp + ddot) + (bp + 2 * U * p) * (np.abs(dp) + s)


def ce_dp_error(y, p, bp, weights):
    """-w y is one rounding, the division one, and 1 / clip(p) moves by bp / p relative (0 where the entry is clipped away)"""
    dp = ce_dp(y, p, weights)
    return np.abs(dp) * (bp / np.maximum(p, LO) + 3 * U)


def upward_error(p, bp):
    """how far above its reference a probability next to 1 can come out.  Its class holds the row's maximum, so its exponential is
    expf(0) = 1 exactly and p' = fl(fl(1 / fl(1 + sum_k e_k')) 1): 1 - p' is (1 - p) moved by the relative errors of the OTHER
    classes' exponentials (at most the largest bp_k / p_k among them, rho; an underflowed one adds 2^-126), and the three additions,
    the reciprocal and the product add 5 U: (1 - p) rho + 5 U.  Never more than bp itself."""
    live = p >= 1e-30
    rho = np.where(live, bp / np.maximum(p, 1e-30), 0.0).max(-1, keepdims=True)
    return np.minimum(bp, SECOND_ORDER * ((1 - p) * rho + 5 * U) + 4 * TINY)


def hi_term(y, p, bp, weights):
    """Within 2^-23 of 1 float32 cannot resolve on which side of the upper clip bound hi = 1 - 2^-23 a probability lies.  Where a
    labelled p_c could come out above hi (p_c + upward_error >= hi) one answer for the pixel's dz row is 0 and the other the row formed
    inside the interval.  Formed by the device at p_c = hi that row is p_c (fl(-w y / p_c) - fl(dot)): the exact difference is
    2^-23 w_c y_c and the two roundings are half an ulp of w_c y_c each, at most 2^-22 w_c y_c in all, and |dz_k| = p_k w_c y_c is
    below that.  Formed by the reference (the device came out above hi) it is the share of the reference's row that the flagged
    entries have when the upper bound is ignored (dz is linear in dp), w_c y_c (1 - p_c), where 1 - p_c <= 2^-23 + upward_error
    is at most 7 U (1 + rho): 1.75 (1 + rho) of the first.  The larger of the two is carried as an absolute term per contributing
    pixel; nothing measurable in the loss."""
    flag = (y != 0) & (p + upward_error(p, bp) >= HI)
    device = 2.0 ** -22 * (flag * np.abs(w64(weights) * y.astype(np.float64))).sum(-1, keepdims=True)
    return np.maximum(device, np.abs(dz_of(p, flag * ce_dp(y, p, weights, hi=2.0))))


def dlogits_ref(dz, shape, loss_scale):
    n, h, w, fy, fx = shape
    return loss_scale * down(dz.reshape(n, h * fy, w * fx, 4), axis_weights(h, fy), axis_weights(w, fx))


def dlogits_bound(dz, ddz, shape, loss_scale):
    """dlogits = sum over the window of (wy wx loss_scale) dz: the per-pixel errors ddz pass through with the reference weights; wy wx
    and its product with loss_scale are two roundings and the chain of K fused multiply-adds gamma(K) (the x8 kernel folds four
    shorter chains with three additions: no longer); with a factor that is no power of two each weight carries axis_weight_error.
    Below the normal range (2^-126) a product is rounded absolutely, or flushed: + 2^-126, as in softmax_bound (a pixel of a saturated
    row under dice has dz near 1e-45, and with a factor of 1 nothing larger joins it in the window)"""
    n, h, w, fy, fx = shape
    wy, wx, dy, dx = axis_weights(h, fy), axis_weights(w, fx), axis_weight_error(h, fy), axis_weight_error(w, fx)
    a = np.abs(dz).reshape(n, h * fy, w * fx, 4)
    out = down(ddz.reshape(a.shape), wy, wx) + gamma(window_terms(h, w, fy, fx) + 3) * down(a, wy, wx)
    if dy.any() or dx.any():
        out = out + down(a, dy, wx) + down(a, wy, dx) + down(a, dy, dx)
    return SECOND_ORDER * abs(loss_scale) * out + TINY


def ce_backward(case, weights, loss_scale, **rule):
    """(dlogits, bound) of the cross-entropy; rule: lo, hi, clip_rule passed to ce_dp (the CPU file's structural errors)"""
    y, p, bp = case["y"], case["p"], case["bp"]
    dz = dz_of(p, ce_dp(y, p, weights, **rule))
    ddz = dz_bound(p, bp, ce_dp(y, p, weights), ce_dp_error(y, p, bp, weights)) + hi_term(y, p, bp, weights)
    return dlogits_ref(dz, case["shape"], loss_scale), dlogits_bound(dz, ddz, case["shape"], loss_scale)


def dice_backward(case, weights, squared, loss_scale):
    """(dlogits, bound) of dice / dice_square: dp_c = fma(A_c, y_c, B_c t_c), t = 1 or 2 p: the coefficients' errors, the product
    B t (one rounding, and 2 bp of t when squared) and the fused multiply-add"""
    y, p, bp = case["y"], case["p"], case["bp"]
    _, coef = dice_ref(y, p, weights, squared)
    dcoef = dice_coef_error(y, p, bp, weights, squared)
    dp = dice_dp(y, p, coef, squared)
    t = 2 * p if squared else np.ones_like(p)
    ddp = (dcoef[:, None, :4] * np.abs(y) + dcoef[:, None, 4:] * t + (np.abs(coef[:, None, 4:]) * 2 * bp if squared else 0.0)
           + 2 * U * (np.abs(coef[:, None, :4] * y) + np.abs(coef[:, None, 4:] * t)))
    dz = dz_of(p, dp)
    return dlogits_ref(dz, case["shape"], loss_scale), dlogits_bound(dz, dz_bound(p, bp, dp, ddp), case["shape"], loss_scale)


# ------------------------------------------------------------------------------------------------- pinned cases
PINNED_LOGITS = (40.0, 0.0, 0.0, 0.0)
PINNED_SHAPES = [(2, 17, 33, 4, 4), (2, 9, 17, 8, 8), (1, 4, 3, 3, 5)]


def pinned_case(shape, cls):
    """constant logits (40, 0, 0, 0), every pixel labelled `cls`.  cls 1: p = e^-40 / (1 + 3 e^-40) = 4e-18 is below lo; cls 0:
    p = 1 - 1.3e-17 rounds to 1, above hi.  Either way every dlogits element is exactly 0 and the loss is npix w_cls (-log bound) within the bound of the sum."""
    n, h, w, fy, fx = shape
    logits = np.broadcast_to(np.asarray(PINNED_LOGITS, F32), (n, h, w, 4)).copy()
    y = np.zeros((n, h * fy * w * fx, 4), F32)
    y[..., cls] = 1.0
    p, bp = prob_ref(logits, fy, fx, "clip" if pow2(fy) and pow2(fx) else "nonpow2")
    # every blend of equal corners returns the corner, expf(0) is 1, and 1 + 3 e^-40 rounds to 1, as does its reciprocal: p_0 is
    # exactly 1 (the GPU file asserts it), so the loss of class 0 carries no error of p
    bp[..., 0] = 0.0
    return dict(logits=logits, y=y, p=p, bp=bp, seed=0, family="pinned", shape=shape)
