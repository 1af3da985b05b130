"""Named edge cases, float64 references and derived error bounds for the kernels that run after the convs: plain NumPy.

The entry points are ssdseg_dice_loss (csrc/losses.hip), ssdseg_metric_mask_iou (csrc/mask_head.hip), ssdseg_metric_label_accuracy,
ssdseg_metric_box_iou, ssdseg_head_gather, ssdseg_softmax_rows (csrc/heads.hip), ssdseg_gap_fwd / _bwd and the pixel sum behind
ssdseg_bilinear_bwd from a 1 x 1 source (csrc/resize.hip), ssdseg_channel_shuffle, ssdseg_channel_gather, ssdseg_copy2d and
ssdseg_copy2d_batch (csrc/shuffle.hip).  tests/test_cpu_tail_cases.py vets the references, the cases and the bounds on the CPU;
tests/test_gpu_tail_edges.py runs the kernels on the same cases.  Every builder seeds its own generator from its arguments, so the
same call gives the same arrays in both files.

U = 2^-24 is the unit roundoff of float32, ULP = 2^-23.  A float32 chain of L roundings over non-negative (or absolute) terms is
within gamma(L) = L U / (1 - L U) of their sum; the chain lengths come from the launch mirrors below.
"""
import numpy as np

from oracle import np_ops as O

F32 = np.float32
U = 2.0 ** -24
ULP = 2.0 ** -23
TINY = 2.0 ** -126                      # smallest normal float32: below it a result is rounded absolutely, or flushed
CW = (0.05, 0.575, 0.135, 0.24)         # the product's class weights of the mask head
CW_ZERO = (0.05, 0.0, 0.71, 0.24)       # one class without weight
LW = (0.0, 1 / 3, 1 / 3, 1 / 3)         # the product's label weights
STDS = (0.1, 0.1, 0.2, 0.2)
KEPS32 = float(F32(1e-7))               # the device's epsilon
LO32 = F32(1e-7)
HI32 = F32(1.0) - F32(1e-7)
CLIP_EDGES = np.array([0.0, 1.0, 5e-8, LO32, np.nextafter(LO32, F32(0)), np.nextafter(LO32, F32(1)),
                       1.0 - 5e-8, HI32, np.nextafter(HI32, F32(0)), np.nextafter(HI32, F32(1))], F32)
ACTS = (O.ACT_NONE, O.ACT_RELU, O.ACT_RELU6, O.ACT_ZERO)
ACT_NAMES = {O.ACT_NONE: "none", O.ACT_RELU: "relu", O.ACT_RELU6: "relu6", O.ACT_ZERO: "zero"}
SECOND_TRIP = 8192 * 256                # work items from which a grid-stride kernel takes a second trip
SECOND_ORDER = 1.01                     # the bounds are first order in U; the largest chain has gamma < 1e-4, its square < 1 % of it


def w64(weights):
    """host weights as the float64 values of the float32 numbers the C-ABI receives"""
    return np.asarray(weights, F32).astype(np.float64)


def gamma(length):
    return length * U / (1.0 - length * U)


def seeded(*key):
    return np.random.default_rng([1993] + [int(k) for k in key])


def one_hot_rows(rng, shape):
    return np.eye(4, dtype=F32)[rng.integers(0, 4, shape)]


def softmax_rows32(rng, shape, sigma=1.5):
    return O.softmax(rng.normal(0, sigma, tuple(shape) + (4,))).astype(F32)


def graded_probs(rng, y):
    """probabilities for the targets y (n, pixels, 4) whose agreement with y depends on the 256-pixel block a pixel is in: the
    ratios I / T of dice and Jaccard do not move when a representative share of the pixels is lost, so no share is representative"""
    group = (np.arange(y.shape[1]) // 256) % 64
    boost = 2.0 * ((group * 40503 >> 3) & 1)          # a strong or a weak prediction, by a hash of the 256-pixel group
    return O.softmax(rng.normal(0, 1.5, y.shape) + boost[None, :, None] * y).astype(F32)


# ------------------------------------------------------------------------------------------------- views
def view_params(c, seed):
    rng = seeded(77, c, seed)
    return rng.uniform(0.5, 1.5, c).astype(F32), rng.uniform(-1.0, 3.0, c).astype(F32)


def gather_view_params(c, seed):
    """scale and a shift that no activation maps to 0: a padded gather entry that received act(shift) would show"""
    s, t = view_params(c, seed)
    return s, (np.abs(t) + F32(0.25)).astype(F32)


def view_ref(x, scale, shift, act, channel=None):
    """act(s x + t) in float64 and the magnitude |s x| + |t| its one rounding is relative to; `channel` maps the last axis of x
    to the entries of scale / shift (default: identity)"""
    x = np.asarray(x, np.float64)
    if scale is None:
        return O.act_fwd(x, act), np.abs(x) * 0.0
    s, t = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    if channel is not None:
        s, t = s[channel], t[channel]
    return O.act_fwd(s * x + t, act), np.abs(s * x) + np.abs(t)


# ------------------------------------------------------------------------------------------------- dice / cross-entropy
DICE_SHAPES = [(1, 1), (2, 255), (2, 256), (1, 2048), (1, 2049), (3, 4100), (1, 131072), (1, 133121), (65, 300)]
DICE_MODES = (0, 1, 2)


def dice_launch(hw):
    """mirror of ssdseg_dice_loss: blocks per image, trips of a thread"""
    nblk = min((hw + 2047) // 2048, 64)
    return dict(nblk=nblk, trips=-(-hw // (nblk * 256)))


def dice_case(n, hw, kind="random"):
    """kind: 'random' | 'absent' (image 0: class 3 absent from y, p exactly 0 there) | 'clip' (p cycles through CLIP_EDGES, soft y)"""
    rng = seeded(1, n, hw)
    y = one_hot_rows(rng, (n, hw))
    p = graded_probs(rng, y)
    if kind == "absent":
        cls = y[0].argmax(-1)
        y[0] = np.eye(4, dtype=F32)[np.where(cls == 3, 0, cls)]
        p[0, :, 3] = 0.0
    elif kind == "clip":
        p = CLIP_EDGES[(np.arange(n * hw * 4) * 7 % CLIP_EDGES.size)].reshape(n, hw, 4).copy()
        y = rng.integers(0, 3, (n, hw, 4)).astype(F32) * F32(0.5)
    return y, p


def dice_sums(y, p, mode):
    """float64 (I_c, T_c) per image: mode 0 sum y p, sum (y + p); 1: squares in T; 2: I = -sum y log(clip p), T unused"""
    y64, p64 = y.astype(np.float64), p.astype(np.float64)
    if mode == 2:
        logp = np.log(np.clip(p, LO32, HI32).astype(np.float64))      # the clip is exact in float32 on both sides
        return -(y64 * logp).sum(axis=1), np.abs(y64 * logp).sum(axis=1)
    inter = (y64 * p64).sum(axis=1)
    return inter, ((y64 * y64 + p64 * p64) if mode == 1 else (y64 + p64)).sum(axis=1)


def dice_ref(y, p, weights, mode):
    w = w64(weights)
    if mode == 2:
        return (dice_sums(y, p, 2)[0] * w).sum(-1)
    return O.dice_loss(y.astype(np.float64)[:, :, None], p.astype(np.float64)[:, :, None], w, squared=bool(mode))


def dice_bound(y, p, weights, mode):
    """Chain: `trips` additions in a thread, 8 tree levels, nblk in the finish kernel, plus the roundings that form a term (mode 0:
    y + p; mode 1: y^2, p^2 and their sum; mode 2: logf at 1 ulp = 2 U and the product).  Closed form per class, r = (2 I + e) / (T + e):
    |dr| <= r (g_I + g_T + 3 U [e added twice, the quotient] + 2 U e / (T + e) [float32 e against the oracle's 1e-7]); 1 - r and its
    product with w are two roundings of |1 - r|; the four terms are added in float32: 4 U of their absolute sum."""
    w = np.abs(w64(weights))
    la = dice_launch(y.shape[1])
    chain = la["trips"] + 8 + la["nblk"]
    inter, total = dice_sums(y, p, mode)
    if mode == 2:
        terms = w * total                   # sum |y log p|
        return SECOND_ORDER * (gamma(chain + 3) * terms.sum(-1) + 5 * U * terms.sum(-1))
    g = gamma(chain + (3 if mode == 1 else 1))
    r = (2 * inter + KEPS32) / (total + KEPS32)
    dr = r * (2 * g + 3 * U + 2 * U * KEPS32 / (total + KEPS32))
    return SECOND_ORDER * ((w * (dr + 2 * U * np.abs(1 - r))).sum(-1) + 4 * U * (w * np.abs(1 - r)).sum(-1))


def drop_block(hw, nblk, q):
    """pixel indices that remain when partial block q of nblk (grid-stride over 256-thread blocks) is lost"""
    i = np.arange(hw)
    return i[(i // 256) % nblk != q]


# ------------------------------------------------------------------------------------------------- soft Jaccard of the masks
IOU_PROB_SHAPES = [(1, 1, 1), (2, 1, 257), (1, 32, 64), (1, 1, 2049), (1, 256, 512), (1, 1, 133121), (65, 3, 5)]
IOU_LOGIT_SHAPES = [(1, 1, 1, 1, 1), (2, 1, 1, 8, 8), (1, 3, 5, 2, 8), (2, 2, 1, 4, 4), (1, 91, 92, 4, 4)]
LOGIT_MAG = 6.0


def iou_launch(npix):
    """mirror of partial_blocks(npix, 64) in csrc/mask_head.hip"""
    nblk = max(1, min((npix + 2047) // 2048, 64))
    return dict(nblk=nblk, trips=-(-npix // (nblk * 256)))


def iou_targets(rng, n, npix):
    """one-hot targets; image 0 has a pixel without any class and (from 8 pixels on) no pixel of class 2"""
    y = one_hot_rows(rng, (n, npix))
    if npix >= 8:
        cls = y[0].argmax(-1)
        y[0] = np.eye(4, dtype=F32)[np.where(cls == 2, 1, cls)]
    y[0, 0] = 0.0
    return y


def iou_prob_case(n, h, w):
    rng = seeded(2, n, h, w)
    y = iou_targets(rng, n, h * w)
    return y, graded_probs(rng, y)


def iou_logit_case(n, h, w, fy, fx):
    rng = seeded(3, n, h, w, fy, fx)
    logits = rng.uniform(-LOGIT_MAG, LOGIT_MAG, (n, h, w, 4)).astype(F32)
    p = O.softmax(O.bilinear_fwd(logits.astype(np.float64), fy, fx)).reshape(n, h * fy * w * fx, 4)
    return iou_targets(rng, n, h * fy * w * fx), logits, p


def iou_ref(y, p, weights):
    return O.metric_mask_iou(y[:, :, None], np.asarray(p, np.float64)[:, :, None], w64(weights))


def logits_prob_error(mag):
    """relative error of softmax(bilinear(logits)) formed in float32, |logit| <= mag, factors that are powers of two (so the blend
    fractions are exact): a lerp a + (b - a) f is a difference (U 2 mag) and a fused multiply-add (U mag), 3 U mag; the second level
    passes the first level's error on (a convex combination) and adds its own: 6 U mag per logit.  a = z - max carries two of those
    and one rounding of at most 2 mag: 14 U mag on the argument of expf, i.e. relative on its value; expf as built adds U |a| <= 2 U mag
    (the uncompensated rounding of a log2(e) under -ffp-contract=fast, see softmax_bound) and the exp2's 1 ulp = 2 U.  A probability is e_c / sum e: twice that, 3 roundings
    of the sum, the reciprocal, the product."""
    return (2 * (16 * mag + 2) + 5) * U


def iou_bound(y, p, weights, perr=0.0):
    """I is a chain of fused multiply-adds, T of (y + p) rounded and added: gamma over trips + 8 + nblk (+ 1).  D = T - I + e >= T / 2
    (t p <= (t + p) / 2 on [0, 1]): no cancellation, |dD| <= dT + dI + 2 U D, so I / D moves by (I / D) (dI / I + dD / D + U); the
    product with w and the float32 sum of the four terms add 5 U of the weighted sum.  perr: relative error of every p."""
    w = np.abs(w64(weights))
    la = iou_launch(y.shape[1])
    g = gamma(la["trips"] + 8 + la["nblk"] + 1)
    y64, p64 = y.astype(np.float64), np.asarray(p, np.float64)
    inter, total = (y64 * p64).sum(1), (y64 + p64).sum(1)
    d_inter, d_total = (g + perr) * inter, g * total + perr * p64.sum(1)
    den = total - inter + KEPS32
    q = inter / den
    dq = d_inter / den + q * ((d_total + d_inter) / den + 3 * U)
    return SECOND_ORDER * ((w * dq).sum(-1) + 5 * U * (w * q).sum(-1))


# ------------------------------------------------------------------------------------------------- label accuracy
ACC_SHAPES = [(1, 1), (2, 255), (2, 256), (3, 257), (1, 150000)]
TIE_ROWS = [(0.25, 0.25, 0.25, 0.25), (0.1, 0.4, 0.1, 0.4), (0.1, 0.1, 0.4, 0.4)]      # maxima at {0,1,2,3}, {1,3}, {2,3}
TIE_FIRST = [0, 1, 2]


def accuracy_case(b, a):
    """random rows; every image starts with the three tie rows (target: the first maximum) and three special target rows
    (all zero, soft, -0.0); with a == 1 the one row is the {1, 3} tie"""
    rng = seeded(4, b, a)
    t, p = one_hot_rows(rng, (b, a)), softmax_rows32(rng, (b, a))
    if a == 1:
        p[:, 0], t[:, 0] = TIE_ROWS[1], np.eye(4, dtype=F32)[1]
        return t, p, np.array([0])
    for k, (row, first) in enumerate(zip(TIE_ROWS, TIE_FIRST)):
        p[:, k], t[:, k] = row, np.eye(4, dtype=F32)[first]
    t[:, 3], t[:, 4], t[:, 5] = 0.0, (0.5, 0.5, 0.0, 0.0), -0.0
    return t, p, np.arange(3)


def accuracy_counts(t, p, last=False):
    """(b, 4) integer counts of equal(one_hot(argmax p), t); last: the LAST maximum instead of the first"""
    am = (3 - p[..., ::-1].argmax(-1)) if last else p.argmax(-1)
    return (np.eye(4, dtype=F32)[am] == t).sum(axis=1)


def accuracy_ref(t, p, weights):
    return O.metric_label_accuracy(t, p, w64(weights))


def accuracy_bound(t, p, weights):
    """the counts are integers below 2^24: exact.  count / a and its product with w are two roundings, the float32 sum of the four
    terms three more of at most their absolute sum: 5 U sum_c |count_c / a w_c|"""
    return 5 * U * (accuracy_counts(t, p) / t.shape[1] * np.abs(w64(weights))).sum(-1)


# ------------------------------------------------------------------------------------------------- box IoU
BOX_SIZES = [1, 255, 256, 257, 9600]
BOX_IMAGES = ("none", "one", "all", "edges")


def box_anchors(a):
    rng = seeded(5, a)
    return (np.round(rng.uniform(40, 600, a)).astype(F32), np.round(rng.uniform(40, 440, a)).astype(F32),
            rng.uniform(20, 300, a).astype(F32), rng.uniform(20, 300, a).astype(F32))


def box_case(a):
    """four images: no object | one object | every anchor an object | edge rows.  Targets of objects have offsets 2 and 3 in
    [0.5, 3] (positive true areas, |o sigma| <= 1.2): a row whose two areas are both 0 has the denominator e - I with I = O(U |c| h),
    a quotient float32 arithmetic does not determine; like the expf overflow corner it is the reference's own and not pinned.
    Edge rows, cyclic over the anchors: 0 perfect prediction, 1 target (2^-140, 0, 0, 0) (an object), 2 target (-0.0, 0, 0, 0)
    (background), 3 predicted width and height clamped at 0 (an intersection extent is at most either box's extent, so such a row
    has I = 0 and q = 0 with or without the clamp: the clamp cannot show in the value, only a NaN or a negative area could), 4 boxes that touch (intersection extent 0.5 with the +1, 0 without),
    5 disjoint boxes, 6 random."""
    rng = seeded(6, a)
    cx, cy, w, h = box_anchors(a)

    def objects(count):
        t = rng.normal(0, 2, (count, 4)).astype(F32)
        t[:, 2:] = rng.uniform(0.5, 3.0, (count, 2)).astype(F32)
        return t
    t = np.zeros((4, a, 4), F32)
    p = rng.uniform(0, 6, (4, a, 4)).astype(F32)
    t[1, a // 2] = objects(1)[0]
    t[2], t[3] = objects(a), objects(a)
    kind = np.arange(a) % 7
    p[3, kind == 0] = t[3, kind == 0]
    t[3, kind == 1] = (2.0 ** -140, 0, 0, 0)
    t[3, kind == 2] = (-0.0, 0, 0, 0)
    p[3, kind == 3, 2:] = F32(-1.0)
    for k, gap in ((4, 0.5), (5, 5.0)):      # predicted box of the true size, its left edge `gap` right of the true right edge
        rows = kind == k
        tw = (np.exp(t[3, rows, 2].astype(np.float64) * float(F32(STDS[2]))) - 1.0) * w[rows]
        p[3, rows] = t[3, rows]
        p[3, rows, 0] = (t[3, rows, 0] + (tw - 1.0 + gap) / (float(F32(STDS[0])) * w[rows])).astype(F32)
    return t, p, (cx, cy, w, h), kind


def box_ref(t, p, anchors, plus_one=1.0, clamp=True, denormal_is_object=True):
    """O.metric_box_iou; the switches restate it with one convention removed (for the CPU vetting only)"""
    sd = w64(STDS)
    if plus_one == 1.0 and clamp and denormal_is_object:
        return O.metric_box_iou(t, p, *anchors, sd)
    return box_terms(t, p, anchors, plus_one, clamp, denormal_is_object)["value"]


def box_terms(t, p, anchors, plus_one=1.0, clamp=True, denormal_is_object=True):
    """the per-anchor quantities of metric_box_iou in float64 with their first-order float32 error bounds (see box_bound)"""
    t64, p64 = np.asarray(t, np.float64), np.asarray(p, np.float64)
    cx, cy, w, h = (np.asarray(v, np.float64) for v in anchors)
    sd = w64(STDS)
    mag = np.abs(t64).sum(-1)
    nb = ((mag > 0) if denormal_is_object else (mag >= TINY)).astype(np.float64)

    def dec(o):
        out = {}
        for ax, (k, c0, size) in enumerate(((0, cx, w), (1, cy, h))):
            arg = o[..., 2 + k] * sd[2 + k]
            ex = np.exp(arg)
            raw = (ex - 1.0) * size
            ext = (np.maximum(0.0, raw) if clamp else raw) * nb
            # the argument, expf as built (U |arg|, see softmax_bound) and its exp2 at 1 ulp; the difference, the product
            e_ext = (size * ex * (2 * np.abs(arg) + 2) * U + 2 * U * np.abs(raw)) * nb
            mid = (o[..., k] * sd[k] * size + c0) * nb
            e_mid = 3 * U * (np.abs(o[..., k] * sd[k] * size) + np.abs(c0)) * nb         # two products and the sum
            lo, hi = (mid - (ext - 1) / 2) * nb, (mid + (ext - 1) / 2) * nb
            e_lo = e_mid + e_ext / 2 + U * np.abs(ext - 1) + U * np.abs(lo)
            e_hi = e_mid + e_ext / 2 + U * np.abs(ext - 1) + U * np.abs(hi)
            out[ax] = (lo, hi, ext, e_lo, e_hi, e_ext)
        return out
    P, T = dec(p64), dec(t64)
    ov, e_ov = [], []
    for ax in (0, 1):
        raw = np.minimum(T[ax][1], P[ax][1]) - np.maximum(T[ax][0], P[ax][0])
        ov.append(np.maximum(0.0, raw + plus_one) * nb)
        e_ov.append((np.maximum(T[ax][4], P[ax][4]) + np.maximum(T[ax][3], P[ax][3]) + 2 * U * (np.abs(raw) + np.abs(raw + plus_one))) * nb)
    inter = ov[0] * ov[1]
    e_inter = ov[0] * e_ov[1] + ov[1] * e_ov[0] + U * inter
    areas = P[0][2] * P[1][2], T[0][2] * T[1][2]
    e_area = sum(b[0][2] * b[1][5] + b[1][2] * b[0][5] + U * a_ for b, a_ in zip((P, T), areas))
    den = areas[0] + areas[1] - inter + KEPS32
    e_den = e_area + e_inter + 3 * U * (areas[0] + areas[1] + inter)
    q = inter / den
    e_q = e_inter / np.abs(den) + np.abs(q) * e_den / np.abs(den) + U * np.abs(q)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(nb=nb, q=q, e_q=e_q, den=den, e_den=e_den, inter=inter, value=q.sum(-1) / nb.sum(-1))


def box_bound(t, p, anchors):
    """Per anchor, first order: the centre c = o s w + c0 is two products and a sum (3 U of |o s w| + |c0|); the extent
    (expf(o s) - 1) w carries the rounding of the argument and the error of expf as built (U |o s| each, relative on the
    exponential; see softmax_bound), the exp2's 1 ulp, the difference
    and the product; a corner c -+ (ext - 1) / 2 adds the roundings of ext - 1 and of the corner; an intersection extent the worse
    corner of each side and two roundings; the products and the denominator theirs; the quotient q = I / D moves by
    dI / D + q dD / D + U q.  The clamps are continuous and never enlarge an error.  The sum over the anchors is a chain of
    ceil(a / 256) additions and 8 tree levels; the count is an exact integer; the final quotient one rounding."""
    terms = box_terms(t, p, anchors)
    a = t.shape[1]
    chain = gamma(-(-a // 256) + 8)
    with np.errstate(invalid="ignore", divide="ignore"):
        count = terms["nb"].sum(-1)
        return SECOND_ORDER * ((chain * np.abs(terms["q"]).sum(-1) + terms["e_q"].sum(-1)) / count + U * np.abs(terms["value"]))


# ------------------------------------------------------------------------------------------------- head gather / softmax
# (b, cells, c, off, total) in anchors of 4 values: image elements in = cells * c, out = total * 4, offset = off * 4
GATHER_SHAPES = [(1, 1, 4, 0, 1), (3, 20, 24, 7, 200), (2, 5, 16, 0, 20), (2, 6, 8, 36, 48), (2, 1048580, 4, 0, 1048580)]


def head_gather_ref(x, scale, shift, act, off, total):
    """(b, cells, c) -> the (b, total, 4) rows a forward head_gather writes, a mask of the written rows, the rounding magnitude"""
    b, cells, c = x.shape
    val, mag = view_ref(x, scale, shift, act)
    n = cells * c // 4
    out, m = np.zeros((b, total, 4)), np.zeros((b, total, 4))
    out[:, off:off + n], m[:, off:off + n] = val.reshape(b, n, 4), mag.reshape(b, n, 4)
    written = np.zeros((b, total, 4), bool)
    written[:, off:off + n] = True
    return out, written, m


SOFTMAX_ROWS = [1, 255, 256, 257, SECOND_TRIP + 1]
SOFTMAX_SPREADS = [0.0, 1e-3, 30.0, 200.0]


def softmax_case(rows, spread, offset=0.0):
    """row 0 has four equal logits, row 1 (if any) the full spread (0, -spread, -spread / 2, -spread) on top of `offset`"""
    rng = seeded(8, rows, int(spread * 1000))
    z = (rng.uniform(-1, 0, (rows, 4)) * spread + offset).astype(F32)
    z[0] = F32(offset)
    if rows > 1:
        z[1] = (F32(offset), F32(offset) - F32(spread), F32(offset) - F32(spread / 2), F32(offset) - F32(spread))
    return z


def softmax_ref(z):
    return O.softmax(np.asarray(z, np.float64))


def softmax_bound(z, zerr=0.0):
    """Roundings of one probability p_c = e_c / sum e, counted: e_c = expf(a), a = z_c - max, has the rounding of a (U |a|, which is
    relative on the value), the error of expf itself, and twice the error `zerr` of a logit that is itself computed; the sum
    inherits the p-weighted mean of these and adds 3 roundings (three additions); the reciprocal 1, the product 1: relative
    (eps_c + sum_k p_k eps_k + 5 U), eps_k = U (2 |z_k - max| + 2) + 2 zerr.  Below the normal range (2^-126) expf may flush and the
    product rounds absolutely: + 2^-126.

    expf itself: the compiler expands it as PH = fl(a log2(e)), PL = fma(a, log2(e), -PH) + a c2 (the rounding of PH and the low
    part of the constant), E = rndne(PH), exp2((PH - E) + PL) 2^E: 1 ulp, which is what ocml documents.  This library is built with
    -ffp-contract=fast, and under it PH - E is contracted into fma(a, log2(e), -E), which no longer carries the rounding of PH; PL,
    added on top, now ADDS that rounding instead of removing it.  The result is off by up to half an ulp of a log2(e) in the
    exponent, ln(2) U |a log2(e)| = U |a| on the value (measured on an MI355X with exact arguments: 5.6 U for |a| < 10, 21 U at
    20 - 40, 43 U from 44 to 88, in steps at the binades of a log2(e); 0.7 - 1.2 U from the same source with contraction off).  The
    bound counts what the built code does: U |a| for that, 2 U for the exp2.  DESIGN.md section 4 has the open item."""
    z64 = np.asarray(z, np.float64)
    p = softmax_ref(z64)
    eps = U * (2 * np.abs(z64 - z64.max(-1, keepdims=True)) + 2) + 2 * zerr
    return SECOND_ORDER * p * (eps + (p * eps).sum(-1, keepdims=True) + 5 * U) + TINY


# ------------------------------------------------------------------------------------------------- average pool / pixel sums
GAP_SHAPES = [(1, 1, 4), (2, 63, 12), (1, 127, 4), (3, 128, 8), (1, 1024, 516), (100, 1024, 8), (600, 1024, 4), (1, 1050, 16), (2, 1200, 576)]
GAP_CHUNKS = [1, 1, 1, 2, 16, 8, 1, 15, 16]
BILINEAR_1X1_SHAPES = [(2, 8, 2, 2), (2, 256, 4, 4), (1, 12, 30, 40)]
GAP_BWD_SHAPES = [(1, 1, 4), (2, 63, 12), (1, 4100, 2048)]


def pixel_sum_launch(n, hw, c, accumulate=0, pitched_out=False):
    """mirror of pixel_sum in csrc/resize.hip"""
    cv = c // 4
    bx = min(cv, 128)
    chunks = next((k for k in range(16, 1, -1) if hw % k == 0 and hw // k >= 64 and n * k <= 1024), 1)
    hwc = hw // chunks
    by = max(1, min(512 // bx, hwc))
    one = chunks == 1 and not accumulate and not pitched_out
    kernels = {"gap_fwd_kernel": 1} if one else {"gap_fwd_kernel": 1, "chunk_sum_kernel": 1}
    return dict(chunks=chunks, hwc=hwc, bx=bx, by=by, gy=-(-cv // bx), trips=-(-hwc // by), one_launch=one, kernels=kernels)


def pixel_sum_bound(terms, launch, extra):
    """terms: (n, hw, c) float64 addends.  A thread adds `trips` of them, row 0 folds blockDim.y partial sums, the second stage
    `chunks`; `extra` counts the other roundings on the way (the view's one, the multiplier and its own rounding, accumulate)"""
    return gamma(launch["trips"] + launch["by"] + launch["chunks"] + extra) * np.abs(terms).sum(axis=1)


def gap_case(n, hw, c):
    return seeded(9, n, hw, c).normal(0, 2, (n, hw, c)).astype(F32)


# ------------------------------------------------------------------------------------------------- channel moves
SHUFFLE_SHAPES = [(1, 4, 1), (5, 6, 3), (7, 6, 6), (300, 116, 2), (9100, 232, 2)]


def shuffle_index(c, groups, inverse=False):
    """source channel of every output channel, as shuffle_kernel computes it"""
    k, per = np.arange(c), c // groups
    return (k % per) * groups + k // per if inverse else (k % groups) * per + k // groups


def shuffle_ref(x, groups, inverse=False):
    m, c = x.shape
    if not inverse:
        return O.channel_shuffle(x.reshape(1, 1, m, c), groups).reshape(m, c)
    return O.channel_shuffle(x.reshape(1, 1, m, c), c // groups).reshape(m, c)


def channel_gather_ref(x, table, scale=None, shift=None, act=O.ACT_NONE, base=None):
    """out[:, j] = act(scale[s] x[:, s] + shift[s]), s = table[j] >= 0, else 0 (+ base) in float64; also the rounding magnitude"""
    table = np.asarray(table)
    live = table >= 0
    src = np.where(live, table, 0)
    val, mag = view_ref(np.asarray(x, np.float64)[:, src], scale, shift, act, channel=src)
    val, mag = val * live, mag * live
    if base is not None:
        val = val + np.asarray(base, np.float64)
    return val, mag


def split_tables(c_log=116, widths=(58, 58)):
    """the packed -> padded split tables of ssdseglib/_ops.py SplitGatherOp and their inverses: [(forward, c_out, backward)]"""
    out, off = [], 0
    for wd in widths:
        cp = (wd + 3) // 4 * 4
        fwd = np.array([off + i if i < wd else -1 for i in range(cp)], np.int32)
        bwd = np.array([j - off if off <= j < off + wd else -1 for j in range(c_log)], np.int32)
        out.append((fwd, cp, bwd))
        off += wd
    return out


def gather_tables():
    """name -> (ldi = c_in, table)"""
    sp = split_tables()
    return {
        "identity": (8, np.arange(8, dtype=np.int32)),
        "reversal": (116, np.arange(115, -1, -1, dtype=np.int32)),
        "all-padding": (8, np.full(8, -1, np.int32)),
        "twice": (8, np.array([5, 1, 5, -1, 0, 7], np.int32)),
        "split0": (116, sp[0][0]), "split1": (116, sp[1][0]), "split0-inverse": (60, sp[0][2]), "split1-inverse": (60, sp[1][2]),
        "narrow": (8, np.array([7, -1, 2], np.int32)),
    }


COPY_BLOCKS = [(1, 1, 1, 1), (1, 257, 257, 257), (300, 7, 9, 12), (2050, 1024, 1024, 1024)]     # rows, cols, ldd, lds


def copy2d_ref(dst, src, rows, cols):
    """dst, src: 2-D arrays whose second axis is the pitch; the block copied, everything else left"""
    out = np.array(dst, copy=True)
    out[:rows, :cols] = src[:rows, :cols]
    return out
