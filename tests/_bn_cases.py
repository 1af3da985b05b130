"""Named edge cases and float64 references for the BatchNorm-statistics, view and strided helper kernels: plain NumPy.

The kernels are ssdseg_bn_finalize, ssdseg_channel_stats, ssdseg_bn_apply, ssdseg_bn_bwd_reduce, ssdseg_gview_materialize and
ssdseg_axpby (csrc/bn.hip) and ssdseg_act_bwd (csrc/shuffle.hip).  tests/test_cpu_bn_cases.py vets the references and the cases on
the CPU (against oracle.np_ops and against finite differences); tests/test_gpu_bn_edges.py runs the kernels on the same cases.
Every builder seeds its own generator, so the same call gives the same arrays in both files.

Rounding units used by the bounds: U = 2^-24 is the unit roundoff of float32 (the error of one correctly rounded operation,
relative to its result), ULP = 2^-23 the relative spacing of float32 numbers ("one ulp relative").
"""
import functools

import numpy as np

from oracle import np_ops as O

F32 = np.float32
U = 2.0 ** -24
ULP = 2.0 ** -23
EPS = 1e-3
MOMENTUM = 0.99
ACTS = (O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6, O.ACT_ZERO)
ACT_NAMES = {O.ACT_NONE: "none", O.ACT_RELU: "relu", O.ACT_RELU6: "relu6", O.ACT_ZERO: "zero"}
BAND = 1e-4             # no pre-activation of a mask test lies this close to 0 or to 6
NUDGE_TO = 3e-4         # where an element found inside the band is moved to
MAX_PARTS = 1024        # csrc/bn.hip: cap of the partial rows of the streaming reductions
MAX_BLOCK_Y = 64        # csrc/bn.hip row_launch: the largest blockDim.y, i.e. the longest in-block fp32 fold


# ------------------------------------------------------------------------------------------------- mirrors of the host code
def reduce_rc(nparts, length):
    """channels per block of the partial-row reductions: mirror of reduce_rc in csrc/reduce_parts.h"""
    if nparts < 32:
        return 32
    return 2 if (nparts >= 256 and length < 2048) else 8


def row_launch(m, c):
    """block and grid of the row-streaming reductions: mirror of row_launch in csrc/bn.hip (without its A/B environment cap)"""
    cv = c // 4
    bx = min(cv, 256)
    by = min(512 // bx, MAX_BLOCK_Y)
    want = (m + by * 8 - 1) // (by * 8)
    return dict(cv=cv, bx=bx, by=by, gx=max(1, min(want, MAX_PARTS)), gy=-(-cv // bx))


# ------------------------------------------------------------------------------------------------------------- references
def fold(table):
    """(nparts, 2, c) float32 partial sums -> (2, c): the sums over the rows, accumulated in extended precision"""
    t = np.asarray(table)
    assert t.dtype == F32 and t.ndim == 3 and t.shape[1] == 2
    return t.astype(np.longdouble).sum(axis=0).astype(np.float64)


def finalize_ref(table_f32, count, gamma, beta, eps, momentum, mm, mv, training):
    """ssdseg_bn_finalize in float64 on the same float32 inputs (include/ssdseg.h, csrc/bn.hip bn_finalize_kernel):
    mean = sum / count, var = max(sumsq / count - mean^2, 0) (biased, clamped), invstd = 1 / sqrt(var + eps),
    scale = gamma * invstd, shift = beta - mean * gamma * invstd; the moving statistics move towards mean and towards
    var * count / (count - 1), the Bessel factor only when count > 1.  eps and momentum are the float32 numbers the C-ABI receives.
    training == 0: mean and var are the moving statistics, which stay as they are.
    -> dict of float64 arrays: mean, var, raw_var (before the clamp), invstd, scale, shift, shift_mag, mm, mv (None without)."""
    eps, mom = float(F32(eps)), float(F32(momentum))
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mm = None if mm is None else np.asarray(mm, np.float64)
    mv = None if mv is None else np.asarray(mv, np.float64)
    if training:
        tot = fold(table_f32)
        mean = tot[0] / count
        raw = tot[1] / count - mean * mean
        var = np.maximum(raw, 0.0)
        if mm is not None:
            unbiased = var * count / (count - 1.0) if count > 1 else var
            mm = mm * mom + mean * (1.0 - mom)
            mv = mv * mom + unbiased * (1.0 - mom)
    else:
        mean, var, raw = mm, mv, mv
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * gamma * invstd
    return dict(mean=mean, var=var, raw_var=raw, invstd=invstd, scale=scale, shift=shift, shift_mag=np.abs(beta) + np.abs(mean * scale),
                mm=mm, mv=mv)


def _view64(x, scale, shift, act):
    z = np.asarray(x, np.float64)
    if scale is not None:
        z = np.asarray(scale, np.float64) * z + np.asarray(shift, np.float64)
    return O.act_fwd(z, act)


def bn_apply_ref(x, scale, shift, act, res=None, rscale=None, rshift=None, ract=O.ACT_NONE):
    """out = act(scale * x + shift) (+ ract(rscale * res + rshift)) in float64 -> (out, |first term| + |second term|)"""
    a = _view64(x, scale, shift, act)
    if res is None:
        return a, np.abs(a)
    b = _view64(res, rscale, rshift, ract)
    return a + b, np.abs(a) + np.abs(b)


def preact64(y, scale, shift):
    return np.asarray(scale, np.float64) * np.asarray(y, np.float64) + np.asarray(shift, np.float64)


def boundary_distance(z, act):
    """smallest distance of a pre-activation to a kink of the activation (inf where it has none)"""
    if act == O.ACT_RELU:
        return float(np.abs(z).min())
    if act == O.ACT_RELU6:
        return float(np.minimum(np.abs(z), np.abs(z - 6.0)).min())
    return float("inf")


def bn_bwd_ref(g, y, scale, shift, mean, invstd, act, count):
    """ssdseg_bn_bwd_reduce in float64 from the arrays the kernel is given (scale, shift, mean, invstd as they are on the device):
    dbeta = sum mask * g, dgamma = sum mask * g * xhat with xhat = (y - mean) * invstd and mask = act'(scale * y + shift),
    k1 = -scale * dgamma * invstd / count, k0 = scale * (dgamma * invstd * mean - dbeta) / count.
    abs_b, abs_g: the per-channel sums of |mask * g| and |mask * g * xhat| that the error bound scales with."""
    g, y = np.asarray(g, np.float64), np.asarray(y, np.float64)
    scale, mean, invstd = (np.asarray(a, np.float64) for a in (scale, mean, invstd))
    mg = O.act_mask(preact64(y, scale, shift), act) * g
    mgx = mg * ((y - mean) * invstd)
    db, dg = mg.sum(axis=0), mgx.sum(axis=0)
    return dict(dbeta=db, dgamma=dg, k1=-scale * dg * invstd / count, k0=scale * (dg * invstd * mean - db) / count,
                abs_b=np.abs(mg).sum(axis=0), abs_g=np.abs(mgx).sum(axis=0))


def chain_bound(m, nparts):
    """2 * (ceil(m / nparts) + 64) * U: the relative error, against the sum of absolute terms, of m float32 terms summed as the
    row-streaming kernels do it: one float32 chain of at most ceil(m / nparts) terms per thread, a serial float32 fold over at most
    64 threads, then float64.  (n - 1) * U / (1 - n * U) is the textbook bound for a chain of n; the factor 2 covers the
    denominator and the rounding of a fused multiply-add term."""
    return 2.0 * (-(-m // nparts) + MAX_BLOCK_Y) * U


def bn_bwd_bounds(ref, scale, mean, invstd, count, m, nparts):
    """error bounds of the four outputs of ssdseg_bn_bwd_reduce against bn_bwd_ref.  The sums carry chain_bound; every term of
    dgamma also carries four ulps for xhat, which the kernel forms in float32 (a subtraction and a product: 2 U, allowed 4 ULP).
    The finalize kernel folds the float32 partial rows in float64 and rounds each output once (U of its own magnitude); the
    errors of the sums reach k1 and k0 through their formulas."""
    scale, mean, invstd = (np.abs(np.asarray(a, np.float64)) for a in (scale, mean, invstd))
    cb = chain_bound(m, nparts)
    e_db = cb * ref["abs_b"]
    e_dg = (cb + 4 * ULP) * ref["abs_g"]
    return dict(dbeta=e_db + U * np.abs(ref["dbeta"]), dgamma=e_dg + U * np.abs(ref["dgamma"]),
                k1=scale * invstd * e_dg / count + U * np.abs(ref["k1"]),
                k0=scale * (invstd * mean * e_dg + e_db) / count + U * np.abs(ref["k0"]))


def gview_ref(g, y, scale, shift, k1, k0, act):
    """dy = scale * mask * g + k1 * y + k0 in float64 -> (dy, mask, |scale * mask * g| + |k1 * y| + |k0|)"""
    g, y = np.asarray(g, np.float64), np.asarray(y, np.float64)
    scale, k1, k0 = (np.asarray(a, np.float64) for a in (scale, k1, k0))
    mask = O.act_mask(preact64(y, scale, shift), act)
    a, b = scale * mask * g, k1 * y
    return a + b + k0, mask, np.abs(a) + np.abs(b) + np.abs(k0)


# ------------------------------------------------------------------------------------------------------- finalize cases
FINALIZE_PAIRS = [(1, 1), (1, 4), (31, 20), (32, 20), (33, 5), (127, 24), (255, 24), (256, 24), (257, 7), (1024, 8), (2048, 16),
                  (300, 2052)]


def _bn_params(rng, c):
    return dict(gamma=rng.uniform(0.5, 1.5, c).astype(F32), beta=rng.normal(0, 0.5, c).astype(F32),
                mm0=rng.normal(0, 1, c).astype(F32), mv0=rng.uniform(0.5, 2, c).astype(F32))


def finalize_table(nparts, c):
    """a table whose rows all differ in magnitude: row p = base * (1 + p / nparts), random signs on the sums.  16 samples per row:
    E[x^2] >= 40 / 16 and |mean| <= 10 * 2 / 16, so the variance is positive without the clamp."""
    rng = np.random.default_rng(1000 * nparts + c)
    grow = 1.0 + np.arange(nparts)[:, None] / nparts
    table = np.empty((nparts, 2, c))
    table[:, 0] = rng.choice([-1.0, 1.0], (nparts, c)) * rng.uniform(2, 10, c) * grow
    table[:, 1] = rng.uniform(40, 80, c) * grow
    return dict(table=table.astype(F32), nparts=nparts, c=c, count=16.0 * nparts, training=1, **_bn_params(rng, c))


def _f32_row_sums(x):
    """(rows, n, c) float32 samples -> (rows, 2, c): sum and sum of squares of every row accumulated sample by sample in float32,
    the square through a fused multiply-add, as channel_stats_kernel forms them"""
    x = np.asarray(x, F32)
    s = np.zeros((x.shape[0], x.shape[2]), F32)
    q = np.zeros_like(s)
    for i in range(x.shape[1]):
        v = x[:, i]
        s = (s + v).astype(F32)
        q = (v.astype(np.float64) * v + q).astype(F32)
    return np.stack([s, q], axis=1)


CONSTANTS = (37.5, -1.1, 0.3, 37.5, 2.7, 1e-2, 37.5, 123.456)


def finalize_single_sample():
    """count = 1 (the GAP branch of the ASPP head at batch 1): one row, one sample per channel.  The samples are multiples of 1/8
    below 32, so their squares are exact in float32 and the biased variance is exactly 0."""
    c = 12
    rng = np.random.default_rng(71)
    x = (rng.integers(-255, 256, c) / 8.0).astype(F32)
    table = np.stack([x, x * x])[None].astype(F32)
    return dict(table=table, nparts=1, c=c, count=1.0, training=1, samples=x, **_bn_params(rng, c))


def finalize_constant_channels():
    """4096 samples over 64 rows; the even channels hold one constant each (CONSTANTS), the odd ones Gaussian data.  The float32
    row sums of a constant that is not a short binary fraction round, and E[x^2] - mean^2 comes out a few 1e-8 x^2 either side of 0."""
    c, rows, per = 16, 64, 64
    rng = np.random.default_rng(72)
    x = rng.normal(0.5, 2.0, (rows, per, c)).astype(F32)
    x[:, :, 0::2] = np.asarray(CONSTANTS, F32)
    return dict(table=_f32_row_sums(x), nparts=rows, c=c, count=float(rows * per), training=1, samples=x.reshape(-1, c),
                constant=np.arange(c) % 2 == 0, **_bn_params(rng, c))


def finalize_no_moving():
    case = finalize_table(33, 5)
    case.update(mm0=None, mv0=None)
    return case


def finalize_inference():
    c = 40
    rng = np.random.default_rng(73)
    return dict(table=None, nparts=0, c=c, count=0.0, training=0, **_bn_params(rng, c))


FINALIZE_CASES = {f"table-{p}x{c}": functools.partial(finalize_table, p, c) for p, c in FINALIZE_PAIRS}
FINALIZE_CASES.update({"single-sample": finalize_single_sample, "constant-channels": finalize_constant_channels,
                       "no-moving-statistics": finalize_no_moving, "inference": finalize_inference})


def finalize_case_ref(case):
    return finalize_ref(case["table"], case["count"], case["gamma"], case["beta"], EPS, MOMENTUM, case["mm0"], case["mv0"], case["training"])


# ----------------------------------------------------------------------------------------------------------- row cases
# (m, c, ld): 1 row; cv = 1 (one lane by 64 rows) and m < blockDim.y; cv = 3; a concat slice; many partial rows; cv = 257 (the second
# grid column has one active lane); the MAX_PARTS cap (16400 rows in blocks of 2 x 8 rows want 1025 partial rows)
ROW_GEOMETRIES = [(1, 4, 4), (7, 4, 12), (63, 12, 12), (513, 20, 36), (4099, 96, 160), (300, 1028, 1032), (16400, 1024, 1024)]


def geometry_id(geom):
    return "m{}-c{}-ld{}".format(*geom)


def batch_affine(y, gamma, beta):
    """float32 (scale, shift) of training-mode BatchNorm over the rows of y: oracle.np_ops.bn_train_fwd"""
    _, cache = O.bn_train_fwd(y, gamma, beta, eps=float(F32(EPS)))
    return cache["scale"], cache["shift"]


def stabilise(y, scale_shift):
    """Moves every element of y (in place) whose float64 pre-activation scale * y + shift lies within BAND of 0 or of 6 to NUDGE_TO
    beyond that boundary, on the side it is on.  scale_shift(y) -> the float32 (scale, shift) that go with y; batch statistics move
    with y, so the search repeats until nothing is inside the band.  -> the share of elements that were moved."""
    moved = np.zeros(y.shape, bool)
    for _ in range(8):
        scale, shift = (np.asarray(a) for a in scale_shift(y))
        clean = True
        for at in (0.0, 6.0):
            # candidates from the native-precision pre-activation (it is within 1e-6 of the float64 one), the decision in float64
            r, ch = np.nonzero(np.abs(scale.astype(y.dtype) * y + shift.astype(y.dtype) - y.dtype.type(at)) < 2 * BAND)
            z = scale[ch].astype(np.float64) * y[r, ch] + shift[ch]
            inside = np.abs(z - at) < BAND
            r, ch, z = r[inside], ch[inside], z[inside]
            if r.size:
                clean = False
                target = at + np.where(z >= at, NUDGE_TO, -NUDGE_TO)
                y[r, ch] = ((target - shift[ch]) / scale[ch]).astype(y.dtype)
                moved[r, ch] = True
        if clean:
            return float(moved.mean())
    raise AssertionError("pre-activations still inside the band after 8 passes")


@functools.lru_cache(maxsize=None)
def row_case(m, c, ld):
    """inputs of every row kernel at one geometry: the raw tensor y with its BatchNorm parameters, a gradient g, a residual tensor
    with an affine of its own, and separate pitches for the other operands.  y and res are stabilised against their affines."""
    rng = np.random.default_rng(100003 * m + c)
    y = rng.standard_normal((m, c), F32) * rng.uniform(0.5, 2.0, c).astype(F32) + rng.normal(0.5, 1.0, c).astype(F32)
    gamma = rng.uniform(1.0, 3.0, c).astype(F32)
    beta = rng.normal(1.5, 2.0, c)
    for at in (0.0, 6.0):       # one row has no spread (z = beta there): keep beta itself off the boundaries
        beta = np.where(np.abs(beta - at) < 0.05, at + 0.05, beta)
    beta = beta.astype(F32)
    share = stabilise(y, lambda t: batch_affine(t, gamma, beta))
    res = rng.standard_normal((m, c), F32) * F32(2.0) + F32(1.0)
    rscale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(F32)
    rshift = rng.normal(1.0, 2.0, c).astype(F32)
    rshare = stabilise(res, lambda t: (rscale, rshift))
    g = rng.standard_normal((m, c), F32)
    # pitches: rows of a concat buffer keep their gap, and every other operand gets a pitch of its own
    pitches = (ld, ld + 4, ld + 8) if ld > c else (c, c, c)
    for a in (y, res, g, gamma, beta, rscale, rshift):
        a.setflags(write=False)
    return dict(m=m, c=c, ld=ld, y=y, gamma=gamma, beta=beta, g=g, res=res, rscale=rscale, rshift=rshift,
                nudged=max(share, rshare), pitches=pitches)


# -------------------------------------------------------------------------------------------------------- boundary case
BOUNDARY_VALUES = np.array([-1.0, -0.0, 0.0, 2.0 ** -140, np.nextafter(F32(6), F32(0)), 6.0, np.nextafter(F32(6), F32(7)), 100.0], F32)
BOUNDARY_MASKS = {O.ACT_NONE: [1, 1, 1, 1, 1, 1, 1, 1], O.ACT_RELU: [0, 0, 0, 1, 1, 1, 1, 1], O.ACT_RELU6: [0, 0, 0, 1, 1, 0, 0, 0],
                  O.ACT_ZERO: [0, 0, 0, 0, 0, 0, 0, 0]}
BOUNDARY_OUTPUTS = {O.ACT_NONE: BOUNDARY_VALUES, O.ACT_RELU: np.array([0, 0, 0, 2.0 ** -140, BOUNDARY_VALUES[4], 6, BOUNDARY_VALUES[6], 100], F32),
                    O.ACT_RELU6: np.array([0, 0, 0, 2.0 ** -140, BOUNDARY_VALUES[4], 6, 6, 6], F32), O.ACT_ZERO: np.zeros(8, F32)}


def boundary_case():
    """scale = 1, shift = 0 on an 8 x 8 Latin square of BOUNDARY_VALUES (every channel sees every value); the gradient holds small
    non-zero integers, so sums of it are exact.  -> y, g, index (which boundary value sits at [r][ch])"""
    r, ch = np.indices((8, 8))
    index = (r + ch) % 8
    g = (((3 * r + ch) % 5 + 1) * np.where((r + 2 * ch) % 3 == 0, -1, 1)).astype(F32)
    return dict(y=BOUNDARY_VALUES[index], g=g, index=index, m=8, c=8)


# ------------------------------------------------------------------------------------------------------------- axpby
AXPBY_COEFFS = [(1.0, 0.0), (0.5, 0.0), (1.0, 1.0), (-2.0, 0.25)]


def axpby_ref(a, b, src, dst):
    """a * src + b * dst as the kernel rounds it.  Every coefficient is a power of two (or 0), so each product is exact and the
    only rounding is that of the sum: float32 NumPy arithmetic gives the same bits.  b == 0: the destination is not an operand."""
    assert all(v == 0 or np.log2(abs(v)) % 1 == 0 for v in (a, b))
    if b == 0:
        return F32(a) * src
    return F32(a) * src + F32(b) * dst
