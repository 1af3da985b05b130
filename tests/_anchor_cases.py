"""Named edge cases for the anchor-side kernels (encode, decode, NMS, segmentation suppression) and for Adam: plain NumPy.

Every builder returns `(inputs, property)`: the inputs of one case as a dict of arrays and scalars, and one line that states what
makes the case an edge.  tests/test_cpu_anchor_edge_cases.py runs the oracle on every case and asserts the property, so a case
cannot degenerate unnoticed when a seed changes; tests/test_gpu_anchor_edges.py runs the kernels on the same inputs.  Each builder
seeds its own generator: the same call gives the same arrays in both files.
"""
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STDS = (0.1, 0.1, 0.2, 0.2)
HALF_BELOW = float(np.nextafter(F32(0.5), F32(0)))       # the float32 just under 0.5
SCORE_06 = float(F32(0.6))                               # the float32 a threshold of 0.6 becomes in the C-ABI
SCORE_06_BELOW = float(np.nextafter(F32(0.6), F32(0)))


def golden_anchors(name):
    d = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return d["corners"].astype(F32), d["centroids"].astype(F32)


# ------------------------------------------------------------------------------------------------------------ NMS / decode
def relu6_offsets(rng, shape):
    """head outputs after ReLU6: a normal draw clipped to [0, 6], so exact 0 and exact 6 are common values"""
    return np.clip(rng.normal(1.5, 2.5, shape), 0.0, 6.0).astype(F32)


def centroids_for(a):
    """`a` rows of (center_x, center_y, width, height): the nb03 anchors, repeated when `a` exceeds their 9600"""
    cent = golden_anchors("anchors_nb03")[1]
    reps = -(-a // cent.shape[0])
    return np.ascontiguousarray(np.tile(cent, (reps, 1))[:a])


def softmax32(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(F32)


def inverted(corners):
    """boxes (ymin, xmin, ymax, xmax) whose corners are the wrong way round on some axis"""
    return (corners[..., 0] > corners[..., 2]) | (corners[..., 1] > corners[..., 3])


def nms_saturated(a=9600, c=4, b=2, max_per_class=4, max_total=10, iou_thr=0.025, score_thr=0.05, seed=11):
    rng = np.random.default_rng(seed)
    cent = centroids_for(a)
    offsets, probs = relu6_offsets(rng, (b, a, 4)), softmax32(3 * rng.normal(0, 1, (b, a, c)))
    # what a trained head does on one object: two anchors of one cell fire for the same class, both with a width offset of exactly
    # 0 (corners inverted by one pixel on x) and different heights.  As TF reads them they are the same one-pixel column, the
    # shorter inside the taller (IoU 0.79): the lower score must go.  Read without the swap both have a negative area and stay.
    _, first, inverse = np.unique(cent[:, :2], axis=0, return_index=True, return_inverse=True)
    twins = [(int(d), int(first[inverse.ravel()[d]])) for d in range(a) if first[inverse.ravel()[d]] != d]
    for img in range(b):
        for cl in range(1, c):
            d2, d1 = twins[(37 * (img * c + cl)) % len(twins)]
            offsets[img, d1], offsets[img, d2] = (0, 0, 0, 3.0), (0, 0, 0, 2.5)
            for d, s in ((d1, 0.999999), (d2, 0.999998)):
                probs[img, d] = (1 - s) / (c - 1)
                probs[img, d, cl] = s
    inputs = dict(offsets=offsets, centroids=cent, probs=probs, c=c, max_per_class=max_per_class, max_total=max_total,
                  iou_thr=iou_thr, score_thr=score_thr)
    return inputs, ("ReLU6-saturated offsets: a width or height offset of exactly 0 decodes to corners inverted by one pixel, "
                    "so the min/max swap of the NMS IoU decides suppressions")


def nms_tied(a=9600, c=4, b=2, max_per_class=4, max_total=10, iou_thr=0.5, score_thr=0.05, seed=12):
    rng = np.random.default_rng(seed)
    probs = (np.round(softmax32(3 * rng.normal(0, 1, (b, a, c))) * 16) / 16).astype(F32)
    inputs = dict(offsets=relu6_offsets(rng, (b, a, 4)), centroids=centroids_for(a), probs=probs, c=c, max_per_class=max_per_class,
                  max_total=max_total, iou_thr=iou_thr, score_thr=score_thr)
    return inputs, ("scores are multiples of 1/16: the order inside a class (lowest anchor first) and of the merge (score, anchor, "
                    "class) decides which of several equal scores survives max_per_class and max_total")


def _grid_corners(a, side=4.0, pitch=10.0, per_row=64):
    """`a` disjoint squares (ymin, xmin, ymax, xmax) on a grid: no two overlap, none is degenerate"""
    i = np.arange(a)
    y0, x0 = (i // per_row) * pitch, (i % per_row) * pitch
    return np.stack([y0, x0, y0 + side, x0 + side], axis=1).astype(F32)


def nms_exact_iou_threshold(iou_thr=0.5):
    """(0,0,1,2) against (0,0,1,1): intersection 1, union 2, IoU exactly 0.5 in float32; the comparison is strict"""
    corners = np.array([[[0, 0, 1, 2], [0, 0, 1, 1], [10, 10, 12, 12], [20, 20, 21, 24], [20, 20, 21, 22]]], F32)
    probs = np.zeros((1, 5, 2), F32)
    probs[0, :, 1] = (0.9, 0.8, 0.7, 0.5, 0.75)          # the second pair meets in the other score order
    probs[0, :, 0] = 1 - probs[0, :, 1]
    inputs = dict(corners=corners, probs=probs, c=2, max_per_class=5, max_total=10, iou_thr=iou_thr, score_thr=0.45)
    return inputs, "two pairs of boxes with IoU exactly 0.5: kept at iou_thr = 0.5, suppressed one float32 below it"


def nms_exact_score_threshold(score_thr=SCORE_06):
    corners = _grid_corners(4)[None]
    probs = np.zeros((1, 4, 2), F32)
    probs[0, :, 1] = (0.7, SCORE_06, SCORE_06_BELOW, 0.65)
    probs[0, :, 0] = (0.1, 0.1, 0.1, SCORE_06)
    inputs = dict(corners=corners, probs=probs, c=2, max_per_class=4, max_total=8, iou_thr=0.5, score_thr=score_thr)
    return inputs, "scores exactly float32(0.6): dropped at score_thr = 0.6, kept one float32 below it"


def nms_thread_ties(a=2100):
    """equal scores on disjoint boxes, max_per_class = 1: the lowest anchor must win.  Class 1: anchors i and i + 1024 (one
    thread's first and second anchor); class 2: i and i + 1 (neighbouring threads); class 3: i + 1 and i + 1024 (the lower anchor
    belongs to the HIGHER thread, so a reduction that breaks ties by thread picks the wrong one)"""
    corners = _grid_corners(a)[None].repeat(2, axis=0)
    probs = np.zeros((2, a, 4), F32)
    probs[..., 0] = 0.25
    s = F32(0.8125)
    probs[0, [5, 5 + 1024], 1] = s
    probs[0, [700, 701], 2] = s
    probs[0, [31, 30 + 1024], 3] = s
    probs[1, [1023, 2047], 1] = s                        # the last thread's two anchors
    probs[1, [1024, 1023], 2] = s                        # thread 0's second anchor against the last thread's first
    probs[1, [2048, 1], 3] = s                           # thread 0's third anchor against thread 1's first
    inputs = dict(corners=corners, probs=probs, c=4, max_per_class=1, max_total=4, iou_thr=0.5, score_thr=0.5)
    return inputs, "equal scores at anchors (i, i+1024), (i, i+1), (i+1, i+1024): the lowest anchor index wins in every pairing"


def nms_dry(a=1025, seed=13):
    """3 to 15 candidates per class: every class runs out before max_per_class, max_total exceeds what all classes give"""
    rng = np.random.default_rng(seed)
    c, b = 4, 2
    probs = np.minimum(softmax32(3 * rng.normal(0, 1, (b, a, c))), F32(0.9))
    for img in range(b):
        picks = rng.permutation(a)
        for cl in range(c):
            k = 3 + 4 * cl
            d, picks = picks[:k], picks[k:]
            probs[img, d] = 0.01
            probs[img, d, cl] = rng.uniform(0.95, 0.97, k).astype(F32)
    inputs = dict(offsets=relu6_offsets(rng, (b, a, 4)), centroids=centroids_for(a), probs=probs, c=c, max_per_class=20, max_total=100,
                  iou_thr=0.3, score_thr=0.9)
    return inputs, "every class runs dry before max_per_class = 20 and max_total = 100 > 4 * 20: the tail rows are zero-filled"


def nms_geometry(a, c, max_per_class, max_total, seed=14):
    """the saturated draw at another anchor count or class / limit geometry; image 1 has no score above the threshold (some are
    exactly on it)"""
    rng = np.random.default_rng(seed + a + 7 * c)
    b = 2
    score_thr = 0.3
    probs = softmax32(3 * rng.normal(0, 1, (b, a, c)))
    probs[1] = np.minimum(probs[1], F32(score_thr))
    inputs = dict(offsets=relu6_offsets(rng, (b, a, 4)), centroids=centroids_for(a), probs=probs, c=c, max_per_class=max_per_class,
                  max_total=max_total, iou_thr=0.1, score_thr=score_thr)
    return inputs, f"a = {a}, c = {c}, limits {max_per_class} / {max_total}; image 1 has every score at or below the threshold"


def nms_bound(a=150000, seed=15):
    """the largest anchor count the argument check admits"""
    rng = np.random.default_rng(seed)
    c = 2
    inputs = dict(offsets=relu6_offsets(rng, (1, a, 4)), centroids=centroids_for(a), probs=softmax32(3 * rng.normal(0, 1, (1, a, c))), c=c,
                  max_per_class=4, max_total=8, iou_thr=0.5, score_thr=0.99)
    return inputs, "a = 150000, the admitted bound: the per-anchor state of one class has to fit the workgroup"


def oracle_corners(inputs):
    """the decoded boxes of a case (the oracle's float32 decode), or its hand-built corners"""
    from oracle import np_ops as O
    if "corners" in inputs:
        return inputs["corners"]
    return O.decode_to_corners_pred(inputs["offsets"], inputs["centroids"], STDS).astype(F32)


def oracle_nms(inputs, corners=None, **override):
    from oracle import np_ops as O
    k = {**inputs, **override}
    corners = oracle_corners(inputs) if corners is None else corners
    return O.combined_nms(corners, k["probs"], k["max_per_class"], k["max_total"], k["iou_thr"], k["score_thr"])


# ------------------------------------------------------------------------------------------------------------------ encode
HAND_ANCHORS = np.array([[0, 0, 9, 9], [0, 0, 9, 4], [0, 0, 9, 4], [100, 100, 109, 109], [20, 20, 29, 29]], F32)
HAND_GT = np.array([[1, 0, 0, 9, 4], [2, 200, 200, 210, 210], [3, 20, 20, 29, 29], [1, 21, 21, 28, 28]], F32)
HAND_MATCH = {0.5: [-1, 0, 0, -1, 3], HALF_BELOW: [0, 0, 0, -1, 3]}


def pack_gt(rows_per_image, gmax):
    b = len(rows_per_image)
    gt = np.zeros((b, gmax, 5), F32)
    cnt = np.zeros(b, np.int32)
    for i, rows in enumerate(rows_per_image):
        rows = np.asarray(rows, F32).reshape(-1, 5)
        cnt[i] = rows.shape[0]
        gt[i, :min(gmax, rows.shape[0])] = rows[:gmax]
    return gt, cnt


def encode_hand(thr):
    """duplicate anchors 1 and 2 (the lower is 'the best anchor' of gt 0, its twin is matched only through the threshold);
    gt 1 overlaps nothing; anchor 0 has IoU exactly 0.5 with gt 0; gt 2 and gt 3 share their best anchor 4, whose own best is
    gt 2: the scatter's last writer, gt 3, wins.  Images: the set, its rows reversed, no ground truth"""
    gt, cnt = pack_gt([HAND_GT, HAND_GT[::-1], np.zeros((0, 5))], 4)
    inputs = dict(anchors=HAND_ANCHORS, gt=gt, cnt=cnt, gmax=4, c=4, thr=thr)
    return inputs, "duplicate anchors, a ground truth without overlap, an IoU exactly on the threshold, a shared best anchor"


def random_gt(rng, g, c, hw, lo=6.0):
    """g boxes (label, xmin, ymin, xmax, ymax) inside an image of hw = (height, width), labels in [1, c)"""
    h, w = hw
    bw = np.exp(rng.uniform(np.log(lo), np.log(0.8 * w), g))
    bh = np.exp(rng.uniform(np.log(lo), np.log(0.8 * h), g))
    x0 = rng.uniform(0, np.maximum(w - bw, 1))
    y0 = rng.uniform(0, np.maximum(h - bh, 1))
    return np.stack([rng.integers(1, c, g), x0, y0, np.minimum(x0 + bw, w - 1), np.minimum(y0 + bh, h - 1)], axis=1).astype(F32)


def encode_ragged(c, seed=21):
    """the reference's anchor generator on a 113 x 257 image: most of the 188 anchors come out inverted and overlap nothing, fifteen
    are single pixels.  No box reaches IoU 0.5 with two of them, so the threshold is 0.01 and one ground truth is a one-pixel-high
    strip from one single-pixel anchor to the next: both have IoU 1/65, the lower index is its best anchor, the other is matched
    through the threshold alone; another is large, so its best anchor stays below the threshold"""
    rng = np.random.default_rng(seed + c)
    anchors = golden_anchors("anchors_ragged")[0]
    rows = random_gt(rng, 8, c, (113, 185))
    rows[:, [1, 3]] += 72                                  # right of the strip's second anchor, so that only the strip reaches it
    rows[:, 0] = 1 + np.arange(8) % (c - 1)               # every label of [1, c) occurs
    rows[3, 1:] = (0, 56, 64, 56)
    rows[0, 1:] = (100, 40, 250, 100)                     # two other single-pixel anchors inside, IoU 1/9211 each: below any threshold, step 1 only
    gt, cnt = pack_gt([rows, np.zeros((0, 5)), rows[5::-1]], 8)
    return dict(anchors=anchors, gt=gt, cnt=cnt, gmax=8, c=c, thr=0.01), f"188 anchors (fewer than one block's threads), c = {c}"


def encode_gmax64(seed=22):
    rng = np.random.default_rng(seed)
    anchors = golden_anchors("anchors_nb03")[0]
    gt, cnt = pack_gt([random_gt(rng, g, 4, (480, 640), 16.0) for g in (64, 63, 1, 0)], 64)
    return dict(anchors=anchors, gt=gt, cnt=cnt, gmax=64, c=4, thr=0.5), "gmax = 64, the limit; images with 64, 63, 1 and 0 boxes"


def encode_1025(seed=23):
    rng = np.random.default_rng(seed)
    anchors = np.ascontiguousarray(golden_anchors("anchors_nb03")[0][:1025])
    gt, cnt = pack_gt([random_gt(rng, 8, 4, (480, 640), 16.0), np.zeros((0, 5)), random_gt(rng, 5, 4, (480, 640), 16.0)], 8)
    gt[2, 4, 1:] = anchors[1024]                          # the one anchor of the second pass is a best anchor
    return dict(anchors=anchors, gt=gt, cnt=cnt, gmax=8, c=4, thr=0.5), "1024 + 1 anchors: thread 0 alone makes a second pass"


def encode_far_twin(seed=24):
    """anchor 1030 is a copy of anchor 7: thread 6 holds the copy, thread 7 the original, and a ground truth equal to both must
    take anchor 7 as its best (the lower index sits in the higher thread)"""
    rng = np.random.default_rng(seed)
    anchors = np.ascontiguousarray(golden_anchors("anchors_nb03")[0][:2048])
    big = np.argsort(-(anchors[:, 2] - anchors[:, 0]))[0]
    anchors[7] = anchors[big]
    anchors[1030] = anchors[7]
    rows = random_gt(rng, 4, 4, (480, 640), 16.0)
    rows[1, 1:] = anchors[7]
    gt, cnt = pack_gt([rows, np.zeros((0, 5)), rows[::-1]], 4)
    return dict(anchors=anchors, gt=gt, cnt=cnt, gmax=4, c=4, thr=0.5), "twin anchors 7 and 1030: the best anchor is the lower index, held by the higher thread"


def encode_overfull(seed=25):
    """gt_count beyond gmax: only the first gmax rows exist and count"""
    rng = np.random.default_rng(seed)
    anchors = golden_anchors("anchors_nb03")[0]
    gmax = 8
    gt, cnt = pack_gt([random_gt(rng, gmax, 4, (480, 640), 16.0), random_gt(rng, 2, 4, (480, 640), 16.0), np.zeros((0, 5))], gmax)
    cnt[0] = gmax + 3
    return dict(anchors=anchors, gt=gt, cnt=cnt, gmax=gmax, c=4, thr=0.5), "gt_count[0] = gmax + 3: clamped to gmax"


def encode_cropped(seed=26):
    """boxes as the crop augmentation leaves them: cut by a window, clipped to the image, some one pixel wide or high"""
    rng = np.random.default_rng(seed)
    anchors = golden_anchors("anchors_nb03")[0]
    h, w = 480, 640
    rows = random_gt(rng, 12, 4, (h, w), 16.0)
    rows[:, 1:] = np.round(rows[:, 1:])
    rows[0, 1], rows[0, 3] = 0, 0                          # one pixel wide, on the left edge
    rows[1, 2], rows[1, 4] = h - 1, h - 1                  # one pixel high, on the bottom edge
    rows[2, 1:] = (w - 1, 100, w - 1, 300)                 # one pixel wide, on the right edge
    rows[3, 1:] = (300, 200, 300, 200)                     # a single pixel
    rows[4, 1:] = (0, 0, w - 1, h - 1)                     # the whole image
    rows[5, 1:] = (0, 0, 40, h - 1)                        # a strip clipped on three sides
    gt, cnt = pack_gt([rows, np.zeros((0, 5)), rows[:6]], 16)
    return dict(anchors=anchors, gt=gt, cnt=cnt, gmax=16, c=4, thr=0.5), "boxes clipped to the image, width or height 1 in the +1 convention"


def iou_plus1(anchors, gt):
    """the encoder's IoU matrix (anchors x boxes): pixel-inclusive extents, float32, the oracle's operation order"""
    one = F32(1)
    ax0, ay0, ax1, ay1 = (anchors[:, i, None].astype(F32) for i in range(4))
    gx0, gy0, gx1, gy1 = (gt[None, :, i].astype(F32) for i in range(1, 5))
    area_a = (ay1 - ay0 + one) * (ax1 - ax0 + one)
    area_g = (gx1 - gx0 + one) * (gy1 - gy0 + one)
    inter = np.maximum(F32(0), np.minimum(ax1, gx1) - np.maximum(ax0, gx0) + one) * \
        np.maximum(F32(0), np.minimum(ay1, gy1) - np.maximum(ay0, gy0) + one)
    return inter / (area_a + area_g - inter)


def encode_steps(anchors, gt, thr):
    """(anchors that step 1 matches: the best anchor of a box with IoU > 0; anchors that step 2 matches: best IoU above thr)"""
    iou = iou_plus1(anchors, gt)
    s1 = np.zeros(anchors.shape[0], bool)
    if gt.shape[0]:
        s1[[int(np.argmax(iou[:, g])) for g in range(gt.shape[0]) if iou[:, g].max() > 0]] = True
        s2 = iou.max(axis=1) > F32(thr)
    else:
        s2 = np.zeros(anchors.shape[0], bool)
    return s1, s2


def oracle_encode(inputs, image):
    from oracle import np_ops as O
    g = min(int(inputs["cnt"][image]), inputs["gmax"])
    return O.encode_targets(inputs["anchors"], inputs["gt"][image, :g], inputs["c"], inputs["thr"], STDS)


ENCODE_CASES = {
    "hand-0.5": lambda: encode_hand(0.5),
    "hand-below-0.5": lambda: encode_hand(HALF_BELOW),
    "ragged-c2": lambda: encode_ragged(2),
    "ragged-c4": lambda: encode_ragged(4),
    "ragged-c7": lambda: encode_ragged(7),
    "gmax64": encode_gmax64,
    "a1025": encode_1025,
    "far-twin": encode_far_twin,
    "overfull": encode_overfull,
    "cropped": encode_cropped,
}

NMS_GEOMETRIES = [(1025, 4, 4, 10), (1025, 2, 1, 1), (1025, 7, 3, 5), (1, 4, 4, 10), (5, 4, 4, 10), (1023, 4, 4, 10), (9600, 4, 4, 10)]
NMS_CASES = {
    "saturated": nms_saturated,
    "tied": nms_tied,
    "iou-on-threshold": lambda: nms_exact_iou_threshold(0.5),
    "iou-above-threshold": lambda: nms_exact_iou_threshold(HALF_BELOW),
    "score-on-threshold": lambda: nms_exact_score_threshold(SCORE_06),
    "score-above-threshold": lambda: nms_exact_score_threshold(SCORE_06_BELOW),
    "thread-ties": nms_thread_ties,
    "dry": nms_dry,
    "bound-150000": nms_bound,
    **{f"a{a}-c{c}-{m}-{t}": (lambda a=a, c=c, m=m, t=t: nms_geometry(a, c, m, t)) for a, c, m, t in NMS_GEOMETRIES},
}


# --------------------------------------------------------------------------------------------------- segmentation suppression
GRID = 4096 * 256                 # threads of the widest grid the element-wise kernels launch


def _rows_of(cls):
    """mask probabilities whose arg-max is `cls`: 0.7 on the class, 0.1 elsewhere"""
    m = np.full((cls.size, 4), 0.1, F32)
    m[np.arange(cls.size), cls] = 0.7
    return m


def seg_case(name, seed=31):
    rng = np.random.default_rng(seed)
    if name == "one-pixel-class3":
        npix, rows, mask, what = 1, 1, _rows_of(np.array([3])), "a single pixel, a single row: only class 3 present"
    elif name == "63-ties":
        npix, rows = 63, 255
        mask = _rows_of(rng.integers(0, 1, npix))
        mask[40] = (0.1, 0.3, 0.3, 0.3)                    # three-way tie: class 1
        mask[62] = (0.1, 0.2, 0.35, 0.35)                  # two-way tie on the last pixel: class 2
        what = "fewer pixels than a wave; ties among classes 1..3 go to the first, so class 3 stays absent"
    elif name == "65-all":
        npix, rows = 65, 255
        mask = _rows_of(np.arange(npix) % 4)
        what = "one pixel more than a wave: all four classes present"
    elif name == "257-last-pixel":
        npix, rows = 257, 1
        cls = np.zeros(npix, np.int64)
        cls[-1] = 2
        mask, what = _rows_of(cls), "one pixel more than a block: class 2 only at the very last pixel"
    elif name == "second-pass-last-pixel":
        npix, rows = GRID + 3, 255
        cls = rng.integers(0, 2, npix)
        cls[-1] = 3
        mask, what = _rows_of(cls), "more pixels than the grid has threads: class 3 only at the last pixel, in the second pass"
    elif name == "second-pass-rows":
        npix, rows = 257, GRID + 1
        cls = rng.integers(1, 4, npix)
        mask, what = _rows_of(cls), "more rows than the grid has threads; class 0 absent"
    else:
        raise KeyError(name)
    probs = rng.uniform(0.01, 1, (rows, 4)).astype(F32)
    return dict(mask=np.ascontiguousarray(mask.reshape(1, npix, 4)), probs=probs), what


SEG_CASES = ["one-pixel-class3", "63-ties", "65-all", "257-last-pixel", "second-pass-last-pixel", "second-pass-rows"]
SEG_PRESENT = {"one-pixel-class3": [0, 0, 0, 1], "63-ties": [1, 1, 1, 0], "65-all": [1, 1, 1, 1], "257-last-pixel": [1, 0, 1, 0],
               "second-pass-last-pixel": [1, 1, 0, 1], "second-pass-rows": [0, 1, 1, 1]}


# ---------------------------------------------------------------------------------------------------------------------- Adam
ADAM_BIG = 2048 * 256 * 4 + 6     # six elements more than the widest launch covers in one pass: a second trip and a tail of 2
ADAM_COUNTS = [1, 3, 4, 5, 1031, ADAM_BIG]
ADAM_HYPER = dict(lr=float(F32(1e-2)), b1=float(F32(0.9)), b2=float(F32(0.999)), eps=float(F32(1e-7)))   # the floats the C-ABI receives


def adam_case(count, steps, seed=41):
    """parameters, one gradient per step (magnitudes log-uniform in 1e-6 .. 1e1, random sign, exact zeros among them) and running
    moments that are not zero (the state after earlier steps)"""
    rng = np.random.default_rng(seed + count % 1000)
    p = rng.normal(0, 1, count).astype(F32)
    m = (rng.normal(0, 1e-2, count)).astype(F32)
    v = (rng.uniform(0, 1e-3, count)).astype(F32)
    g = (np.exp(rng.uniform(np.log(1e-6), np.log(1e1), (steps, count))) * rng.choice([-1.0, 1.0], (steps, count))).astype(F32)
    zero = rng.uniform(size=(steps, count)) < 0.1
    zero[0, 0] = False                                      # the first gradient of a one-element case is not zero
    if steps > 1:
        zero[1, -1] = True                                  # an exact zero in the last (tail) element
    g[zero] = 0.0
    return dict(p=p, m=m, v=v, g=g), "gradients over seven decades with exact zeros; count % 4 != 0 runs the tail"


def adam_oracle(inputs, first_step, grad_scale, dtype):
    """the oracle's Adam over the case's gradients in `dtype` -> (p, m, v)"""
    from oracle import np_ops as O
    p, m, v = (inputs[k].astype(dtype) for k in ("p", "m", "v"))
    h = ADAM_HYPER
    for s, g in enumerate(inputs["g"]):
        gs = g.astype(dtype) * dtype(grad_scale)
        p, m, v = O.adam_step(p, gs, m, v, first_step + s, h["lr"], h["b1"], h["b2"], h["eps"])
    return p, m, v
