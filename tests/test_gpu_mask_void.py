"""GPU parity of the void-pixel variants of the mask losses and of the mask metric (through the C-ABI and the public callables) vs the
float64 references of tests/_void_cases.py, which tests/test_cpu_void_cases.py vets.

ssdseg_mask_head_fwd_dice_void / _bwd_dice_void, ssdseg_mask_head_fwd_bootstrap_void / _bwd_bootstrap_void,
ssdseg_bootstrap_ce_loss_void, ssdseg_metric_mask_iou_void (csrc/mask_head.hip) and ssdseg_dice_loss_void (csrc/losses.hip) on the
smallest shapes that reach each backward kernel and its borders -- x4 with one partial tile and with several tiles, x8 with partial
tiles, the gather kernel at x2 and x1, x4 again under SSDSEG_MASK_BWD=gather -- and five void patterns: none, one image entirely
void, a single labelled pixel, a void rectangle with edges on a tile border and on the image border, scattered void pixels.

The bounds are the plain twins' derived bounds evaluated on what the void paths sum (tests/_void_cases.py says why nothing is
added).  Exact claims: a void pixel's stored loss, the L = 0 image's loss (0.0), kept (0) and thresh (+inf), keep and kept as
integers, the gradient of every low-resolution pixel whose window holds no labelled (or kept) pixel (+0, by its bits), the x4 tile
kernel against the gather kernel, and -- with no void pixel -- every output of a _void entry against its plain twin's, bit for bit.

Pinned as they behave today: the cross-entropy ignores void pixels; crop and mosaic with fill_class = 255 give all-zero one-hot
rows in the padding.  Engine level: two train_on_batch steps with the void loss and metric on masks free of void equal the plain
ones bit for bit; with masks entirely void the mask loss is 0.0 and no weight reachable only from the mask head moves.

Run with -s for the largest error / bound ratio of every case.
"""
import ctypes as C

import numpy as np
import pytest

import _mask_cases as MC
import _void_cases as VC
from _guard import guards  # noqa: F401  (fixture)
from _edge_helpers import c4, finish, launched, ratio, reporter, same_bits, untouched

pytestmark = pytest.mark.gpu

F32 = np.float32
CW, SCALE = VC.CW, 0.5
report = reporter("mask-void")


def zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


def backward(ctx, guards, monkeypatch, entry, shape, args, gather=False):
    """dlogits (n, h, w, 4) of a backward entry (args: what follows the head arguments, without the output) and its kernel's name"""
    n, h, w, fy, fx = shape
    g = guards.out((n, h, w, 4))
    if gather:
        monkeypatch.setenv("SSDSEG_MASK_BWD", "gather")
    kernels = launched(ctx, lambda: ctx.call(entry, *args, g))
    if gather:
        monkeypatch.delenv("SSDSEG_MASK_BWD")
    assert untouched(g) == 0 and len(kernels) == 1 and list(kernels.values()) == [1], kernels
    return g.download(), next(iter(kernels))


def backward_paths(ctx, guards, monkeypatch, entry, shape, args, ref, bound, live):
    """the default kernel against float64, the gradient of the low-resolution pixels outside `live` exactly +0; for x4 the gather
    kernel bit for bit, for x8 within the bound"""
    got, name = backward(ctx, guards, monkeypatch, entry, shape, args)
    ratios = {"dlogits": ratio(got, ref, bound)}
    assert zero_bits(got[~live]), "a window without a contributing pixel: the gradient is not +0"
    if shape[3:] in ((4, 4), (8, 8)):
        gat, gname = backward(ctx, guards, monkeypatch, entry, shape, args, gather=True)
        assert gname != name and "mask_head_bwd_kernel" in gname and ("tile" in name)
        assert zero_bits(gat[~live])
        if shape[3] == 4:
            assert same_bits(got, gat), "x4 tile kernel != gather kernel"
        else:
            ratios["gather"] = ratio(gat, ref, bound)
    else:
        assert "mask_head_bwd_kernel" in name
    return ratios, got, name


# ------------------------------------------------------------------------------------------------------- dice / dice_square
def dice_forward(ctx, guards, case, squared, void):
    n, h, w, fy, fx = case["shape"]
    dl, dy = guards.inp(case["logits"]), guards.inp(case["y"])
    prob, loss, coef = guards.out(case["y"].shape), guards.out(n), guards.out((n, 8))
    entry = "ssdseg_mask_head_fwd_dice" + ("_void" if void else "")
    kernels = launched(ctx, lambda: ctx.call(entry, dl, n, h, w, 4, fy, fx, dy, c4(CW), squared, prob, loss, coef))
    assert kernels == {"mask_head_fwd_dice_kernel" + ("<VOID>" if void else ""): 1, "mask_dice_final_kernel": 1}, kernels
    assert untouched(prob) + untouched(loss) + untouched(coef) == 0
    return dl, dy, coef, dict(prob=prob.download(), loss=loss.download(), coef=coef.download())


@pytest.mark.parametrize("squared", (0, 1), ids=("dice", "dice_square"))
@pytest.mark.parametrize("pattern", VC.PATTERNS)
@pytest.mark.parametrize("shape", VC.SHAPES, ids=VC.tag)
def test_dice_void(ctx, guards, monkeypatch, shape, pattern, squared):
    n, h, w, fy, fx = shape
    case = VC.void_case(shape, pattern)
    y, p, bp = case["y"], case["p"], case["bp"]
    lab = VC.labelled(y)
    dl, dy, coef, got = dice_forward(ctx, guards, case, squared, True)
    loss_ref, coef_ref = VC.dice_void_ref(y, p, CW, squared)
    ratios = dict(prob=ratio(got["prob"], p, bp), loss=ratio(got["loss"], loss_ref, VC.dice_void_bound(case, CW, squared)),
                  coef=ratio(got["coef"], coef_ref, VC.dice_void_coef_error(case, CW, squared)))
    for i in range(n):
        if not lab[i].any():
            assert got["loss"][i] == 0.0 and loss_ref[i] == 0.0, "an image without a labelled pixel: the loss is not exactly 0"
    ref, bound = VC.dice_void_backward(case, CW, squared, SCALE)
    args = (dl, n, h, w, 4, fy, fx, dy, coef, squared, SCALE)
    back, dlogits, name = backward_paths(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_dice_void", shape, args, ref, bound, VC.reach(case))
    assert "VOID" in name
    if pattern == "image":
        assert zero_bits(dlogits[min(1, n - 1)]) and (n == 1 or dlogits[0].any())
    if pattern == "none":                                                  # nothing void: the plain entries' bits
        _, _, plain_coef, plain = dice_forward(ctx, guards, case, squared, False)
        assert all(same_bits(got[k], plain[k]) for k in got)
        plain_g, plain_name = backward(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_dice", shape, (dl, n, h, w, 4, fy, fx, dy, plain_coef, squared, SCALE))
        assert same_bits(dlogits, plain_g) and "VOID" not in plain_name
    else:                                                                  # the plain entry is NOT this: void pixels pull its T up
        _, _, _, plain = dice_forward(ctx, guards, case, squared, False)
        assert not same_bits(got["loss"], plain["loss"])
    report("dice void", f"{VC.tag(shape)} {pattern} squared{squared}", **ratios, **back)
    finish(ctx, guards)


# ------------------------------------------------------------------------------------------------------ bootstrapped
BOOT_OUTS = ("prob", "pixel_loss", "thresh", "keep", "kept", "loss")


def bootstrap_forward(ctx, guards, case, fraction, void):
    n, h, w, fy, fx = case["shape"]
    y = case["y"]
    npix = y.shape[1]
    dl, dy = guards.inp(case["logits"]), guards.inp(y)
    outs = dict(prob=guards.out(y.shape), pixel_loss=guards.out((n, npix)), thresh=guards.out(n), keep=guards.out(n, np.int32),
                kept=guards.out(n, np.int32), loss=guards.out(n))
    if void:
        call = lambda: ctx.call("ssdseg_mask_head_fwd_bootstrap_void", dl, n, h, w, 4, fy, fx, dy, c4(CW), float(fraction), outs["prob"],
                                outs["pixel_loss"], outs["thresh"], outs["keep"], outs["kept"], outs["loss"])
    else:
        from ssdseglib import losses as LS
        outs.pop("keep")
        call = lambda: ctx.call("ssdseg_mask_head_fwd_bootstrap", dl, n, h, w, 4, fy, fx, dy, c4(CW), LS.bootstrap_keep(fraction, npix), outs["prob"],
                                outs["pixel_loss"], outs["thresh"], outs["kept"], outs["loss"])
    kernels = launched(ctx, call)
    want = {"bootstrap_hist_kernel": 4, "bootstrap_sum_kernel": 1, "bootstrap_final_kernel": 1}
    want.update({"mask_head_fwd_pixel_void_kernel": 1, "bootstrap_keep_kernel": 1} if void else {"mask_head_fwd_pixel_kernel": 1})
    assert kernels == want, kernels
    assert not any(untouched(b) for b in outs.values())
    return dl, dy, outs, {k: b.download() for k, b in outs.items()}


@pytest.mark.parametrize("fraction", VC.KEEP_FRACTIONS, ids=("0.25", "1.0", "1e-9"))
@pytest.mark.parametrize("pattern", VC.PATTERNS)
@pytest.mark.parametrize("shape", VC.SHAPES, ids=VC.tag)
def test_bootstrap_void(ctx, guards, monkeypatch, shape, pattern, fraction):
    n, h, w, fy, fx = shape
    case = VC.void_case(shape, pattern)
    y, p, bp = case["y"], case["p"], case["bp"]
    lab = VC.labelled(y)
    ref = VC.bootstrap_void_ref(y, p, CW, fraction)
    tb = VC.pixel_loss_bound(case, CW)
    dl, dy, outs, got = bootstrap_forward(ctx, guards, case, fraction, True)
    pl, thresh = got["pixel_loss"], got["thresh"]

    assert np.array_equal(got["keep"], ref["keep"])
    assert same_bits(pl[~lab], np.full(int((~lab).sum()), VC.VOID_LOSS, F32)) and (pl[lab] >= 0).all()
    ratios = dict(prob=ratio(got["prob"], p, bp), pixel=ratio(pl, ref["l"], tb))
    # the selection, on the device's own stored losses: exact
    for i in range(n):
        k = int(got["keep"][i])
        own = np.sort(pl[i][lab[i]])[::-1]
        assert same_bits(thresh[i:i + 1], own[k - 1:k] if k else np.array([np.inf], F32)), (i, thresh[i], k)
    mask_dev = pl >= thresh[:, None]
    assert not (mask_dev & ~lab).any() and np.array_equal(got["kept"], mask_dev.sum(1)) and (got["kept"] >= got["keep"]).all()
    some = ref["keep"] > 0
    ratios["thresh"] = ratio(thresh[some], ref["thresh"][some], (tb * lab).max(1)[some]) if some.any() else 0.0
    # the kept sum and the gradient, with the device's selection
    own_ref = VC.bootstrap_void_ref(y, p, CW, fraction, keep_mask=mask_dev)
    ratios["loss"] = ratio(got["loss"], own_ref["loss"], VC.bootstrap_sum_bound(ref["l"], mask_dev, tb))
    for i in range(n):
        if not lab[i].any():
            assert got["loss"][i] == 0.0 and got["kept"][i] == 0 and got["keep"][i] == 0 and thresh[i] == np.inf
    # against the reference's own selection: only pixels within two bounds of the threshold may differ
    band = lab & (np.abs(ref["l"] - ref["thresh"][:, None]) <= 2 * tb)
    assert not ((mask_dev != ref["mask"]) & ~band).any()

    dref, dbound = VC.bootstrap_void_backward(case, CW, mask_dev, SCALE)
    live = VC.reach(dict(case, y=y * mask_dev[..., None]))
    args = (dl, n, h, w, 4, fy, fx, dy, c4(CW), outs["pixel_loss"], outs["thresh"], SCALE)
    back, dlogits, _ = backward_paths(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_bootstrap_void", shape, args, dref, dbound, live)
    if pattern == "none":                                                  # nothing void: the plain entries' bits, and the host's keep
        from ssdseglib import losses as LS
        assert (got["keep"] == LS.bootstrap_keep(fraction, y.shape[1])).all()
        _, _, plain_outs, plain = bootstrap_forward(ctx, guards, case, fraction, False)
        assert all(same_bits(got[k], plain[k]) for k in plain)
        plain_g, _ = backward(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_bootstrap", shape,
                              (dl, n, h, w, 4, fy, fx, dy, c4(CW), plain_outs["pixel_loss"], plain_outs["thresh"], SCALE))
        assert same_bits(dlogits, plain_g)
    report("bootstrap void", f"{VC.tag(shape)} {pattern} keep{fraction:g}", **ratios, **back)
    finish(ctx, guards)


def test_bootstrap_void_rejects_bad_arguments(ctx, guards):
    from _edge_helpers import rejected
    case = VC.void_case(VC.SHAPES[0], "scattered")
    n, h, w, fy, fx = case["shape"]
    dl, dy = guards.inp(case["logits"]), guards.inp(case["y"])
    pl, thr, keep, kept, loss = guards.out((n, case["y"].shape[1])), guards.out(n), guards.out(n, np.int32), guards.out(n, np.int32), guards.out(n)
    for fraction in (0.0, -0.25, 1.5, float("nan")):
        rejected(ctx, "ssdseg_mask_head_fwd_bootstrap_void", dl, n, h, w, 4, fy, fx, dy, c4(CW), fraction, None, pl, thr, keep, kept, loss)
        rejected(ctx, "ssdseg_bootstrap_ce_loss_void", dy, dy, n, h * fy * w * fx, 4, c4(CW), fraction, loss)
    rejected(ctx, "ssdseg_mask_head_fwd_bootstrap_void", dl, n, h, w, 4, fy, fx, dy, c4(CW), 0.25, None, pl, thr, None, kept, loss)
    rejected(ctx, "ssdseg_mask_head_fwd_bootstrap_void", dl, 65536, h, w, 4, fy, fx, dy, c4(CW), 0.25, None, pl, thr, keep, kept, loss)
    rejected(ctx, "ssdseg_mask_head_fwd_dice_void", dl, 65536, h, w, 4, fy, fx, dy, c4(CW), 0, None, loss, None)
    rejected(ctx, "ssdseg_mask_head_bwd_dice_void", dl, n, h, w, 4, fy, fx, dy, None, 0, 0.5, loss)
    rejected(ctx, "ssdseg_metric_mask_iou_void", dl, 65536, h, w, 4, fy, fx, 1, dy, c4(CW), loss)
    rejected(ctx, "ssdseg_dice_loss_void", dy, dy, n, 4, 4, c4(CW), 2, loss)
    assert untouched(pl) == pl.size and untouched(loss) == loss.size and untouched(keep) == keep.size
    finish(ctx, guards)


@pytest.mark.parametrize("shape", VC.SHAPES, ids=VC.tag)
def test_without_void_pixels_the_plain_bits_off_the_lattice(ctx, guards, monkeypatch, shape):
    """normal logits (every rounding of the up-sampling and the softmax is live, as in training) and labels free of void: every
    output of every _void entry has the bits of its plain twin"""
    n, h, w, fy, fx = shape
    y = MC.TC.one_hot_rows(VC.seeded(77, *shape), (n, h * fy * w * fx))
    case = dict(logits=MC.mask_logits(shape, "normal", 0), y=y, shape=shape)
    for squared in (0, 1):
        dl, dy, coef, got = dice_forward(ctx, guards, case, squared, True)
        _, _, plain_coef, plain = dice_forward(ctx, guards, case, squared, False)
        assert all(same_bits(got[k], plain[k]) for k in got), f"dice squared{squared}"
        g, _ = backward(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_dice_void", shape, (dl, n, h, w, 4, fy, fx, dy, coef, squared, SCALE))
        pg, _ = backward(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_dice", shape, (dl, n, h, w, 4, fy, fx, dy, plain_coef, squared, SCALE))
        assert same_bits(g, pg) and g.any()
    for fraction in VC.KEEP_FRACTIONS:
        dl, dy, outs, got = bootstrap_forward(ctx, guards, case, fraction, True)
        _, _, plain_outs, plain = bootstrap_forward(ctx, guards, case, fraction, False)
        assert all(same_bits(got[k], plain[k]) for k in plain), f"bootstrap {fraction}"
        g, _ = backward(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_bootstrap_void", shape,
                        (dl, n, h, w, 4, fy, fx, dy, c4(CW), outs["pixel_loss"], outs["thresh"], SCALE))
        pg, _ = backward(ctx, guards, monkeypatch, "ssdseg_mask_head_bwd_bootstrap", shape,
                         (dl, n, h, w, 4, fy, fx, dy, c4(CW), plain_outs["pixel_loss"], plain_outs["thresh"], SCALE))
        assert same_bits(g, pg) and g.any()
    void_m, plain_m = guards.out(n), guards.out(n)
    ctx.call("ssdseg_metric_mask_iou_void", dl, n, h, w, 4, fy, fx, 1, dy, c4(CW), void_m)
    ctx.call("ssdseg_metric_mask_iou", dl, n, h, w, 4, fy, fx, 1, dy, c4(CW), plain_m)
    assert same_bits(void_m.download(), plain_m.download()) and void_m.download().all()
    finish(ctx, guards)


# --------------------------------------------------------------------------------------------- metric, standalone callables
@pytest.mark.parametrize("pattern", VC.PATTERNS)
@pytest.mark.parametrize("shape", VC.SHAPES, ids=VC.tag)
def test_metric_void(ctx, guards, shape, pattern):
    """both paths of ssdseg_metric_mask_iou_void: from the logits (the training step) and from given probabilities"""
    n, h, w, fy, fx = shape
    case = VC.void_case(shape, pattern)
    y, p, bp = case["y"], case["p"], case["bp"]
    lab = VC.labelled(y)
    dl, dy = guards.inp(case["logits"]), guards.inp(y)
    out = guards.out(n)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_metric_mask_iou_void", dl, n, h, w, 4, fy, fx, 1, dy, c4(CW), out))
    assert kernels == {"mask_iou_partial_kernel<true, VOID>": 1, "mask_iou_finish_kernel": 1}, kernels
    from_logits = out.download()
    perr = float((bp / p).max())                                           # the relative error of every probability
    ratios = dict(logits=ratio(from_logits, VC.iou_void_ref(y, p, CW), VC.iou_void_bound(y, p, CW, perr)))
    p32 = p.astype(F32)
    dp, out2 = guards.inp(p32), guards.out(n)
    kernels = launched(ctx, lambda: ctx.call("ssdseg_metric_mask_iou_void", dp, n, h * fy, w * fx, 4, 1, 1, 0, dy, c4(CW), out2))
    assert kernels == {"mask_iou_partial_kernel<false, VOID>": 1, "mask_iou_finish_kernel": 1}, kernels
    from_prob = out2.download()
    ratios["prob"] = ratio(from_prob, VC.iou_void_ref(y, p32, CW), VC.iou_void_bound(y, p32, CW))
    for i in range(n):
        if not lab[i].any():
            assert from_logits[i] == 0.0 and from_prob[i] == 0.0
    plain_l, plain_p = guards.out(n), guards.out(n)
    ctx.call("ssdseg_metric_mask_iou", dl, n, h, w, 4, fy, fx, 1, dy, c4(CW), plain_l)
    ctx.call("ssdseg_metric_mask_iou", dp, n, h * fy, w * fx, 4, 1, 1, 0, dy, c4(CW), plain_p)
    if pattern == "none":
        assert same_bits(from_logits, plain_l.download()) and same_bits(from_prob, plain_p.download())
    elif (lab.any(1) & ~lab.all(1)).any():                                 # an image with both kinds of pixel: the plain metric is NOT this
        assert not same_bits(from_logits, plain_l.download()) and not same_bits(from_prob, plain_p.download())
    report("metric void", f"{VC.tag(shape)} {pattern}", **ratios)
    finish(ctx, guards)


@pytest.mark.parametrize("pattern", VC.PATTERNS)
def test_standalone_callables(ctx, guards, pattern):
    """losses.dice / dice_square / bootstrapped_cross_entropy and metrics.jaccard_iou_segmentation_masks called directly with
    ignore_void=True run the _void entries on given probabilities"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    shape = (3, 17, 18, 4, 4)
    n, h, w, fy, fx = shape
    case = VC.void_case(shape, pattern)
    y = case["y"]
    lab = VC.labelled(y)
    p32 = case["p"].astype(F32)
    y4, p4 = y.reshape(n, h * fy, w * fx, 4), p32.reshape(n, h * fy, w * fx, 4)
    ratios = {}
    for squared, factory in enumerate((ssdseglib.losses.dice, ssdseglib.losses.dice_square)):
        got = factory(CW, ignore_void=True)(y4, p4)
        want = VC.dice_void_ref(y, p32.astype(np.float64), CW, squared)[0]
        ratios[factory.__name__] = ratio(got, want, VC.dice_loss_void_bound(y, p32, CW, squared))
        assert got.shape == (n,) and all(got[i] == 0.0 for i in range(n) if not lab[i].any())
        if pattern == "none":
            assert same_bits(got, factory(CW)(y4, p4))
    got = ssdseglib.metrics.jaccard_iou_segmentation_masks(CW, ignore_void=True)(y4, p4)
    ratios["jaccard"] = ratio(got, VC.iou_void_ref(y, p32, CW), VC.iou_void_bound(y, p32, CW))
    if pattern == "none":
        assert same_bits(got, ssdseglib.metrics.jaccard_iou_segmentation_masks(CW)(y4, p4))
    # bootstrapped: the given float32 probabilities are exact inputs (bp = 0); the selection is checked where it is visible
    # (test_bootstrap_void), here the loss against the reference whose selection no pixel is within two bounds of
    exact = dict(case, p=p32.astype(np.float64), bp=np.zeros_like(case["bp"]))
    tb = VC.pixel_loss_bound(exact, CW)
    for fraction in VC.KEEP_FRACTIONS:
        ref = VC.bootstrap_void_ref(y, exact["p"], CW, fraction)
        gap = np.abs(ref["l"] - ref["thresh"][:, None])
        decided = ~(lab & (gap <= 2 * tb) & (gap > 0)).any(1)              # (a pixel AT the threshold is a tie both sides keep)
        got = ssdseglib.losses.bootstrapped_cross_entropy(CW, fraction, ignore_void=True)(y4, p4)
        bound = VC.bootstrap_sum_bound(ref["l"], ref["mask"], tb)
        assert decided.any() or not lab.any()
        ratios[f"bootstrap{fraction:g}"] = ratio(got[decided], ref["loss"][decided], bound[decided])
        assert all(got[i] == 0.0 for i in range(n) if not lab[i].any())
        if pattern == "none":
            assert same_bits(got, ssdseglib.losses.bootstrapped_cross_entropy(CW, fraction)(y4, p4))
    report("standalone void", pattern, **ratios)
    finish(ctx, guards)


# ------------------------------------------------------------------------------------ pinned: cross-entropy, fill_class = 255
def test_cross_entropy_ignores_void_as_it_stands(ctx, guards):
    """x1, so that a pixel's probabilities are its own logits': moving the logits behind void pixels moves neither the loss nor
    the gradient of any labelled pixel, and a void pixel's gradient row is zero; the standalone callable likewise"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    shape = (2, 3, 5, 1, 1)
    n, h, w, fy, fx = shape
    case = VC.void_case(shape, "scattered")
    y = case["y"]
    lab = VC.labelled(y).reshape(n, h, w)
    moved = case["logits"].copy()
    moved[~lab] = MC.lattice(VC.seeded(75), moved[~lab].shape, 6.0)
    assert (~lab).any() and not np.array_equal(moved, case["logits"])
    results = []
    for logits in (case["logits"], moved):
        dl, dy = guards.inp(logits), guards.inp(y)
        prob, loss, g = guards.out(y.shape), guards.out(n), guards.out((n, h, w, 4))
        ctx.call("ssdseg_mask_head_fwd", dl, n, h, w, 4, fy, fx, dy, c4(CW), prob, loss)
        ctx.call("ssdseg_mask_head_bwd", dl, n, h, w, 4, fy, fx, dy, c4(CW), SCALE, g)
        p4 = prob.download().reshape(n, h, w, 4)
        results.append((loss.download(), g.download(), ssdseglib.losses.cross_entropy(CW)(y.reshape(n, h, w, 4), p4), p4))
    (l0, g0, s0, p0), (l1, g1, s1, p1) = results
    assert not np.array_equal(p0, p1) and same_bits(p0[lab], p1[lab])
    assert same_bits(l0, l1) and same_bits(g0, g1) and same_bits(s0, s1) and l0.all()
    assert not g0[~lab].any() and g0[lab].any()
    finish(ctx, guards)


def test_fill_class_255_is_void_after_the_expand(ctx, guards):
    """a zoom-out crop window and a mosaic whose tiles zoom out, fill_class = 255, at 8 x 12: the class indices are the host spec's,
    and after ssdseg_expand_inputs the one-hot rows of the padding are all zero exactly, every other row one-hot"""
    from ssdseglib import datacoder as D
    b, h, w = 2, 8, 12
    rng = VC.seeded(76)
    idx = rng.integers(0, 4, (b, h, w)).astype(np.uint8)
    p_idx = guards.inp(idx, dtype=np.uint8)
    windows = np.array([[-6, -4, 24, 16], [0, 0, w, h]], np.float32)                     # sample 0: the image in the middle of twice its size
    index4 = np.array([[0, 1, 1, 0], [1, 0, 0, 1]], np.int32)
    split = np.array([[5, 3], [w, h]], np.int32)
    tiles = np.array([[[-3, -2, 12, 8], [0, 0, w, h], [2, -4, 8, 16], [0, 0, 6, 4]], [[0, 0, w, h]] * 4], np.float32)
    cases = {}
    d_idx = guards.out((b, h, w), np.uint8)
    ctx.call("ssdseg_crop_inputs", None, p_idx, b, None, windows.ctypes.data_as(C.POINTER(C.c_float)), None, 255, None, None, None, d_idx, b, h, w)
    cases["crop"] = (d_idx, D._crop_resample(None, idx, windows, (0, 0, 0), 255)[1])
    m_idx = guards.out((b, h, w), np.uint8)
    ctx.call("ssdseg_mosaic_inputs", None, p_idx, b, index4.ctypes.data, split.ctypes.data, tiles.ctypes.data_as(C.POINTER(C.c_float)), None, 255,
             None, None, None, m_idx, b, h, w)
    cases["mosaic"] = (m_idx, D._mosaic_resample(None, idx, D.Mosaic(index4, split, tiles), (0, 0, 0), 255)[1])
    for name, (dev, want) in cases.items():
        got = dev.download()
        assert np.array_equal(got, want), name
        pad = got == 255
        assert pad[0].any() and not pad[0].all() and not pad[1].any() and set(np.unique(got)) <= {0, 1, 2, 3, 255}, name
        onehot = guards.out((b, h, w, 4))
        ctx.call("ssdseg_expand_inputs", None, dev, None, None, onehot, b, h, w, 4)
        rows = onehot.download()
        assert zero_bits(rows[pad]) and np.array_equal(rows[~pad], np.eye(4, dtype=F32)[got[~pad]]), name
    finish(ctx, guards)


# ------------------------------------------------------------------------------------------------------------ engine level
def compiled(seed, void):
    import ssdseglib
    from tests.test_gpu_full_model import CW as MODEL_CW, build
    boxes, _, model = build(seed=seed)
    model.compile(optimizer=ssdseglib.optimizers.SGD(learning_rate=1e-2),
                  loss={'output-mask': ssdseglib.losses.dice(MODEL_CW, ignore_void=True) if void else ssdseglib.losses.dice(MODEL_CW),
                        'output-labels': ssdseglib.losses.confidence_loss, 'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights={'output-mask': 1.0, 'output-labels': 1.0, 'output-boxes': 1.0},
                  metrics={'output-mask': ssdseglib.metrics.jaccard_iou_segmentation_masks(MODEL_CW, ignore_void=True) if void
                           else ssdseglib.metrics.jaccard_iou_segmentation_masks(MODEL_CW)})
    return boxes, model


def weights_of(model):
    return {(l.name, name): value for l in model.layers for name, value in zip(l.weights, l.get_weights())}


def test_train_steps_with_the_void_loss_and_metric(ctx):
    """(a) masks free of void: two train_on_batch steps with dice(w, ignore_void=True) and the void metric give the plain ones'
    losses, metrics and weights bit for bit.  (b) masks entirely void: the mask loss is exactly 0.0, no trainable weight reachable
    only from the mask head moves, and the detection losses are those of (a)'s first step"""
    from ssdseglib import _engine as E
    from tests.test_gpu_full_model import SHAPE, make_targets
    E.set_default_context(ctx)
    rng = np.random.default_rng(1993)
    runs = {}
    for void in (False, True):
        boxes, model = compiled(7, void)
        if not runs:
            x = rng.integers(0, 256, (2,) + SHAPE).astype(np.float32)
            _, _, targets = make_targets(rng, boxes, 2)
            assert VC.labelled(targets['output-mask']).all()
        logs = [model.train_on_batch(x, targets) for _ in range(2)]
        runs[void] = (logs, weights_of(model))
        assert all(np.isfinite(v) for step in logs for v in step.values())
    (plain_logs, plain_w), (void_logs, void_w) = runs[False], runs[True]
    assert plain_logs == void_logs and plain_logs[0] != plain_logs[1]
    assert plain_w.keys() == void_w.keys() and all(same_bits(plain_w[k], void_w[k]) for k in plain_w)

    boxes, model = compiled(7, True)
    before = weights_of(model)
    empty = dict(targets, **{'output-mask': np.zeros_like(targets['output-mask'])})
    logs = model.train_on_batch(x, empty)
    after = weights_of(model)
    assert logs['output-mask_loss'] == 0.0 and logs['output-mask_jaccard_iou_segmentation_masks_metric'] == 0.0
    assert logs['output-labels_loss'] == plain_logs[0]['output-labels_loss'] and logs['output-boxes_loss'] == plain_logs[0]['output-boxes_loss']
    head = [k for k in before if k[0].startswith("mask-") and not k[1].startswith("moving_")]
    assert len(head) > 20 and all(same_bits(before[k], after[k]) for k in head)
    moved = [k for k in before if not k[0].startswith("mask-") and not k[1].startswith("moving_") and not same_bits(before[k], after[k])]
    assert moved, "the detection losses moved nothing: the step did not run"
    # the plain dice on the same void masks is not 0: every probability counts against T
    boxes, model = compiled(7, False)
    assert model.train_on_batch(x, empty)['output-mask_loss'] != 0.0
