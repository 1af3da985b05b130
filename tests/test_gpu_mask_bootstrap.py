"""GPU parity of the bootstrapped cross-entropy of the mask head (`ssdseg_mask_head_fwd_bootstrap` / `_bwd_bootstrap`,
`ssdseg_bootstrap_ce_loss`): the kernels against the fp64 oracle of tests/_bootstrap_oracle.py (pinned by
test_cpu_bootstrap_oracle.py), against the cross-entropy entry points bit for bit where every pixel is kept, and the engine /
Keras surface on top.

The parity test is decomposed so that no pixel near the threshold can hide or fake a failure: the per-pixel losses against the
oracle within B, the threshold / count / sum against the device's OWN downloaded pixel losses exactly, the gradient against the
oracle's gradient taken with the device's keep mask, and the device's keep mask against the oracle's own with every difference
inside the band |l_ref - tau_ref| <= 2 B.  B = 8 x the largest difference between the oracle and the same oracle functions run
on float32 arrays, computed per case on the CPU (3.3e-7 ... 7.1e-7 before the factor): the factor covers logf against the
correctly rounded log, and contraction."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import np_ops as O
from oracle.np_model import NpModel
import _bootstrap_oracle as B
from _guard import guards  # noqa: F401  (fixture)
from tests.test_gpu_backbone import device_relu_masks, rel
from tests.test_gpu_full_model import CW, SHAPE, build, make_targets
from tests.test_gpu_head_ops import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(2, 12, 16), (1, 17, 35), (3, 5, 3)]      # whole 16x16 tiles; ragged tiles; fewer pixels than one block
CW32 = np.asarray(CW, np.float32)
CW64 = CW32.astype(np.float64)
NEW_ENTRIES = ("ssdseg_mask_head_fwd_bootstrap", "ssdseg_mask_head_bwd_bootstrap", "ssdseg_bootstrap_ce_loss")
FWD_OUTS = ("prob", "pixel_loss", "thresh", "kept", "loss")


def c4(w):
    return (C.c_float * 4)(*[float(v) for v in w])


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def head_case(n, h, w, f):
    """test_mask_head's inputs, drawn in its order, and what every test of the case shares (read-only): the fp64 references, the
    float32 restatement of the pixel losses, and B"""
    rng = np.random.default_rng(1993)
    logits = rng.normal(0, 2, (n, h, w, 4)).astype(np.float32)
    cls = rng.integers(0, 4, (n, h * f, w * f))
    y = np.eye(4, dtype=np.float32)[cls]
    p_ref = O.softmax(O.bilinear_fwd(logits.astype(np.float64), f, f))
    l_ref = B.pixel_losses(y.astype(np.float64), p_ref, CW64)
    l32 = B.pixel_losses(y, O.softmax(O.bilinear_fwd(logits, f, f)), CW32)
    assert l32.dtype == np.float32
    bound = 8.0 * float(np.abs(l32.astype(np.float64) - l_ref).max())
    return frozen(logits, y, p_ref, l_ref, l32) + (bound,)


def run_fwd(ctx, guards, dl, dy, shape, f, keep, cw=CW32, present=FWD_OUTS):
    n, h, w = shape
    hw = h * f * w * f
    shapes = dict(prob=(n, h * f, w * f, 4), pixel_loss=(n, hw), thresh=(n,), kept=(n,), loss=(n,))
    outs = {k: guards.out(shapes[k], np.int32 if k == "kept" else np.float32) for k in present}
    ctx.call("ssdseg_mask_head_fwd_bootstrap", dl, n, h, w, 4, f, f, dy, c4(cw), keep, *[outs.get(k) for k in FWD_OUTS])
    ctx.sync()
    guards.check()
    for k in present:
        assert guards.unwritten(outs[k]).size == 0, k
    return outs, {k: outs[k].download() for k in present}


def run_bwd(ctx, guards, dl, dy, shape, f, outs, scale=0.5, cw=CW32):
    n, h, w = shape
    g = guards.out((n, h, w, 4))
    ctx.call("ssdseg_mask_head_bwd_bootstrap", dl, n, h, w, 4, f, f, dy, c4(cw), outs["pixel_loss"], outs["thresh"], scale, g)
    ctx.sync()
    guards.check()
    assert guards.unwritten(g).size == 0
    return g.download()


def check_selection(got, keep, y, p_ref, cw64=CW64):
    """1(c)-(e): threshold, count and sum against the device's own pixel losses; the sum against the oracle with the device's mask.
    -> the device's keep mask (n, H*W)"""
    pl, thresh = got["pixel_loss"], got["thresh"]
    n, hw = pl.shape
    kth = np.partition(pl, hw - keep, axis=1)[:, hw - keep]
    assert np.array_equal(bits(thresh), bits(kth)), (thresh, kth)
    keep_dev = pl >= thresh[:, None]
    assert np.array_equal(got["kept"], keep_dev.sum(axis=1)) and (got["kept"] >= keep).all()
    own = np.where(keep_dev, pl.astype(np.float64), 0.0).sum(axis=1)
    want, _ = B.with_keep_mask(y.astype(np.float64), p_ref, cw64, keep_dev)
    print("loss rel err vs own kept sum", rel_err(got["loss"], own), "vs oracle with the device's mask", rel_err(got["loss"], want))
    assert rel_err(got["loss"], own) < 1e-5 and rel_err(got["loss"], want) < 1e-5
    return keep_dev


def dlogits_ref(y, p_ref, keep_dev, f, scale=0.5, cw64=CW64):
    _, dp = B.with_keep_mask(y.astype(np.float64), p_ref, cw64, keep_dev)
    return O.bilinear_bwd(O.softmax_bwd(p_ref, dp * scale), f, f)


# ------------------------------------------------------------------------------------------------ 1. parity, decomposed
@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("f", [4, 8])
@pytest.mark.parametrize("fraction", [0.25, 0.03, None], ids=["0.25", "0.03", "keep1"])
def test_bootstrap_parity(ctx, guards, fraction, f, n, h, w):
    logits, y, p_ref, l_ref, l32, bound = head_case(n, h, w, f)
    hw = h * f * w * f
    keep = 1 if fraction is None else B.keep_count(fraction, hw)
    # (g), the condition on the inputs, from the reference alone
    _, _, mask_ref, tau_ref = B.bootstrapped_cross_entropy(y.astype(np.float64), p_ref, CW64, keep)
    band = np.abs(l_ref - tau_ref[:, None, None]) <= 2 * bound
    mask32 = l32 >= B.thresholds(l32, keep)[:, None, None]
    print(f"B = {bound:.3e} (float32 restatement {bound / 8:.3e}), keep = {keep} of {hw}, pixels in the band: {int(band.sum())}, "
          f"float32 restatement differs from the reference's mask in {int((mask32 != mask_ref).sum())}")
    assert 1 <= band.sum() <= 16

    dl, dy = guards.inp(logits), guards.inp(y)
    outs, got = run_fwd(ctx, guards, dl, dy, (n, h, w), f, keep)
    err_p = float(np.abs(got["prob"] - p_ref).max())
    err_l = float(np.abs(got["pixel_loss"].reshape(l_ref.shape) - l_ref).max())
    print(f"|prob - ref| = {err_p:.3e}, |pixel_loss - ref| = {err_l:.3e} (B = {bound:.3e})")
    assert err_p < 2e-6                                                                        # (a)
    assert err_l <= bound                                                                      # (b)
    keep_dev = check_selection(got, keep, y, p_ref)                                            # (c) (d) (e)
    g = run_bwd(ctx, guards, dl, dy, (n, h, w), f, outs)
    err_g = rel_err(g, dlogits_ref(y, p_ref, keep_dev.reshape(mask_ref.shape), f))
    print(f"dlogits rel err {err_g:.3e}")
    assert err_g < 2e-5                                                                        # (f)
    differs = keep_dev.reshape(mask_ref.shape) != mask_ref                                     # (g)
    print("keep mask differs from the reference's in", int(differs.sum()), "pixels")
    assert not (differs & ~band).any()


# ------------------------------------------------------------------------------ 2. keep = H W is the cross-entropy
@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("f", [4, 8])
def test_keeping_every_pixel_is_the_cross_entropy(ctx, guards, monkeypatch, f, n, h, w):
    logits, y, p_ref, _, _, _ = head_case(n, h, w, f)
    hw = h * f * w * f
    dl, dy = guards.inp(logits), guards.inp(y)
    outs, got = run_fwd(ctx, guards, dl, dy, (n, h, w), f, hw)
    assert (got["kept"] == hw).all() and np.array_equal(got["thresh"], got["pixel_loss"].min(axis=1))
    ce_loss = guards.out(n)
    ctx.call("ssdseg_mask_head_fwd", dl, n, h, w, 4, f, f, dy, c4(CW32), None, ce_loss)
    assert rel_err(got["loss"], ce_loss.download()) < 1e-5
    for path in ("default", "gather"):
        if path == "gather":
            monkeypatch.setenv("SSDSEG_MASK_BWD", "gather")
        g = run_bwd(ctx, guards, dl, dy, (n, h, w), f, outs)
        ce = guards.out((n, h, w, 4))
        ctx.call("ssdseg_mask_head_bwd", dl, n, h, w, 4, f, f, dy, c4(CW32), 0.5, ce)
        assert np.abs(g).max() > 0 and np.array_equal(bits(g), bits(ce.download())), path


# ---------------------------------------------------------------------------------------------------------- 3. ties
def test_every_tied_pixel_is_kept(ctx, guards):
    """all-zero logits: p = 0.25 exactly, so l takes the four values w_c log 4 (class 1 > 3 > 2 > 0 with CW) and keep = 50 falls
    inside class 3 (image 0: 30 + 50 pixels at or above) and inside class 1 (image 1: 60)"""
    n, h, w, f, keep = 2, 5, 3, 4, 50
    hw = h * f * w * f
    rng = np.random.default_rng(1993)
    counts = ({1: 30, 3: 50, 2: 60, 0: 100}, {1: 60, 3: 40, 2: 40, 0: 100})
    cls = np.stack([rng.permutation(np.repeat(list(c), list(c.values()))) for c in counts]).reshape(n, h * f, w * f)
    y = np.eye(4, dtype=np.float32)[cls]
    logits = np.zeros((n, h, w, 4), np.float32)
    p_ref = np.full(y.shape, 0.25)
    dl, dy = guards.inp(logits), guards.inp(y)
    outs, got = run_fwd(ctx, guards, dl, dy, (n, h, w), f, keep)
    assert np.array_equal(got["prob"], p_ref.astype(np.float32))
    pl = got["pixel_loss"].reshape(cls.shape)
    values = [np.unique(pl[cls == c]) for c in range(4)]
    assert all(v.size == 1 for v in values)                            # one float per class
    assert all(abs(float(v[0]) - CW64[c] * np.log(4.0)) <= 1e-6 * CW64[c] * np.log(4.0) for c, v in enumerate(values))
    assert np.array_equal(got["thresh"], np.array([values[3][0], values[1][0]]))
    assert got["kept"].tolist() == [80, 60] and (got["kept"] > keep).all()
    keep_dev = check_selection(got, keep, y, p_ref)
    assert np.array_equal(keep_dev.reshape(cls.shape), np.stack([np.isin(cls[0], (1, 3)), cls[1] == 1]))
    g = run_bwd(ctx, guards, dl, dy, (n, h, w), f, outs)
    assert rel_err(g, dlogits_ref(y, p_ref, keep_dev.reshape(cls.shape), f)) < 2e-5

    # a class with weight 0: l = +0 exactly; with keep = H W the threshold is 0 and everything is kept
    cw0 = np.array([0.0, 0.575, 0.135, 0.24], np.float32)
    outs, got = run_fwd(ctx, guards, dl, dy, (n, h, w), f, hw, cw=cw0)
    assert not bits(got["pixel_loss"].reshape(cls.shape)[cls == 0]).any()
    assert not bits(got["thresh"]).any() and got["kept"].tolist() == [hw, hw]
    keep_dev = check_selection(got, hw, y, p_ref, cw0.astype(np.float64))
    assert keep_dev.all()
    g = run_bwd(ctx, guards, dl, dy, (n, h, w), f, outs, cw=cw0)
    assert rel_err(g, dlogits_ref(y, p_ref, keep_dev.reshape(cls.shape), f, cw64=cw0.astype(np.float64))) < 2e-5


# --------------------------------------------------------------------------------------- 4. per-image independence
@pytest.mark.parametrize("f", [4, 8])
def test_an_image_does_not_depend_on_its_batch(ctx, guards, f):
    n, h, w = 3, 12, 16
    logits, y, _, _, _, _ = head_case(n, h, w, f)
    keep = B.keep_count(0.25, h * f * w * f)
    outs, whole = run_fwd(ctx, guards, guards.inp(logits), guards.inp(y), (n, h, w), f, keep, present=FWD_OUTS[1:])
    whole["dlogits"] = run_bwd(ctx, guards, guards.inp(logits), guards.inp(y), (n, h, w), f, outs)
    for b in range(n):
        dl, dy = guards.inp(logits[b:b + 1]), guards.inp(y[b:b + 1])
        outs, alone = run_fwd(ctx, guards, dl, dy, (1, h, w), f, keep, present=FWD_OUTS[1:])
        alone["dlogits"] = run_bwd(ctx, guards, dl, dy, (1, h, w), f, outs)
        for k, v in alone.items():
            assert np.array_equal(bits(v), bits(whole[k][b:b + 1])), (b, k)


# ------------------------------------------------------------------------------------------- 5. the real key count
def test_select_at_the_real_pixel_count(ctx, guards):
    """one image of 120 x 160 logits x4: 307,200 keys, all four radix passes populated"""
    n, h, w, f = 1, 120, 160, 4
    rng = np.random.default_rng(1993)
    logits = rng.normal(0, 2, (n, h, w, 4)).astype(np.float32)
    y = np.eye(4, dtype=np.float32)[rng.integers(0, 4, (n, h * f, w * f))]
    p_ref = O.softmax(O.bilinear_fwd(logits.astype(np.float64), f, f))
    keep = B.keep_count(0.25, h * f * w * f)
    assert keep == 76800
    _, got = run_fwd(ctx, guards, guards.inp(logits), guards.inp(y), (n, h, w), f, keep, present=FWD_OUTS[1:])
    check_selection(got, keep, y, p_ref)


# ---------------------------------------------------------------------------- 6. dropped pixels are exact zeros
@pytest.mark.parametrize("f", [4, 8])
def test_dropped_pixels_give_bit_zero_gradient_rows(ctx, guards, monkeypatch, f):
    """From one low-resolution column left of the middle on, every logit row is 8 on one class (per image) and the target is that
    class: those pixels have l < 1e-3, the rest of the image is random, and 3 % of the pixels are kept.  All of them lie in the left
    half, and every low-resolution pixel that no kept pixel interpolates from has an all-zero-bits gradient row"""
    n, h, w = 2, 12, 16
    rng = np.random.default_rng(1993)
    logits = rng.normal(0, 2, (n, h, w, 4)).astype(np.float32)
    cls = rng.integers(0, 4, (n, h * f, w * f))
    for b, k in enumerate((1, 3)):
        logits[b, :, w // 2 - 1:] = 8.0 * np.eye(4, dtype=np.float32)[k]
        cls[b, :, (w // 2 - 1) * f:] = k
    y = np.eye(4, dtype=np.float32)[cls]
    keep = B.keep_count(0.03, h * f * w * f)
    dl, dy = guards.inp(logits), guards.inp(y)
    outs, got = run_fwd(ctx, guards, dl, dy, (n, h, w), f, keep, present=FWD_OUTS[1:])
    keep_dev = (got["pixel_loss"] >= got["thresh"][:, None]).reshape(cls.shape)
    assert keep_dev.any(axis=(1, 2)).all() and not keep_dev[:, :, w * f // 2:].any()
    reached = O.bilinear_bwd(np.repeat(keep_dev[..., None].astype(np.float64), 4, axis=-1), f, f) != 0
    assert (~reached).all(axis=-1)[:, :, w // 2 + 1:].all() and reached.any()
    for path in ("default", "gather"):
        if path == "gather":
            monkeypatch.setenv("SSDSEG_MASK_BWD", "gather")
        g = run_bwd(ctx, guards, dl, dy, (n, h, w), f, outs)
        assert not bits(g[~reached]).any(), path
        assert np.abs(g[reached]).max() > 0


# ---------------------------------------------------------------------------------- 7. optional outputs and errors
def test_optional_outputs(ctx, guards):
    """the NULL subsets the engine uses (training: no probabilities; validation / predict-with-loss: all) and the bare minimum:
    what is present is bit-identical to the full call"""
    n, h, w, f = 1, 17, 35, 4
    logits, y, _, _, _, _ = head_case(n, h, w, f)
    keep = B.keep_count(0.25, h * f * w * f)
    dl, dy = guards.inp(logits), guards.inp(y)
    _, full = run_fwd(ctx, guards, dl, dy, (n, h, w), f, keep)
    for present in (("pixel_loss", "thresh", "kept", "loss"), ("pixel_loss", "thresh", "loss"), ("prob", "pixel_loss", "thresh"),
                    ("pixel_loss", "thresh")):
        _, part = run_fwd(ctx, guards, dl, dy, (n, h, w), f, keep, present=present)
        for k in present:
            assert np.array_equal(bits(part[k]), bits(full[k])), (present, k)


def test_bad_arguments_are_errors_before_any_launch(ctx, guards):
    from ssdseglib import _hip as H
    n, h, w, f = 3, 5, 3, 4
    hw = h * f * w * f
    logits, y, _, _, _, _ = head_case(n, h, w, f)
    dl, dy = guards.inp(logits), guards.inp(y)
    o = dict(prob=guards.out(y.shape), pixel_loss=guards.out((n, hw)), thresh=guards.out(n), kept=guards.out(n, np.int32), loss=guards.out(n),
             dlogits=guards.out(logits.shape), alone=guards.out(n))
    outs = [o[k] for k in FWD_OUTS]
    fwd, bwd, alone = NEW_ENTRIES
    bad = [(fwd, dl, n, h, w, 3, f, f, dy, c4(CW), 60, *outs), (fwd, dl, n, h, w, 4, f, f, dy, c4(CW), 0, *outs),
           (fwd, dl, n, h, w, 4, f, f, dy, c4(CW), hw + 1, *outs), (fwd, dl, n, h, w, 4, f, f, dy, c4(CW), -1, *outs),
           (fwd, None, n, h, w, 4, f, f, dy, c4(CW), 60, *outs), (fwd, dl, n, h, w, 4, f, f, None, c4(CW), 60, *outs),
           (fwd, dl, n, h, w, 4, f, f, dy, None, 60, *outs),
           (fwd, dl, n, h, w, 4, f, f, dy, c4(CW), 60, o["prob"], None, o["thresh"], o["kept"], o["loss"]),
           (fwd, dl, n, h, w, 4, f, f, dy, c4(CW), 60, o["prob"], o["pixel_loss"], None, o["kept"], o["loss"]),
           (bwd, dl, n, h, w, 3, f, f, dy, c4(CW), o["pixel_loss"], o["thresh"], 0.5, o["dlogits"]),
           (bwd, dl, n, h, w, 4, f, f, dy, c4(CW), None, o["thresh"], 0.5, o["dlogits"]),
           (bwd, dl, n, h, w, 4, f, f, dy, c4(CW), o["pixel_loss"], None, 0.5, o["dlogits"]),
           (bwd, dl, n, h, w, 4, f, f, dy, c4(CW), o["pixel_loss"], o["thresh"], 0.5, None),
           (alone, dy, o["prob"], n, hw, 3, c4(CW), 60, o["alone"]), (alone, dy, o["prob"], n, hw, 4, c4(CW), 0, o["alone"]),
           (alone, dy, o["prob"], n, hw, 4, c4(CW), hw + 1, o["alone"]), (alone, dy, o["prob"], n, hw, 4, c4(CW), 60, None),
           (alone, None, o["prob"], n, hw, 4, c4(CW), 60, o["alone"])]
    for args in bad:
        with pytest.raises(H.SsdsegError):
            ctx.call(*args)
    ctx.sync()
    guards.check()
    for k, buf in o.items():
        assert len(guards.unwritten(buf)) == buf.download().size, k


# ------------------------------------------------------------------------------------------------- 8. determinism
def test_bootstrap_is_deterministic(ctx, guards):
    n, h, w, f = 1, 17, 35, 8
    logits, y, _, _, _, _ = head_case(n, h, w, f)
    keep = B.keep_count(0.25, h * f * w * f)
    dl, dy = guards.inp(logits), guards.inp(y)
    runs = []
    for _ in range(2):
        outs, got = run_fwd(ctx, guards, dl, dy, (n, h, w), f, keep)
        got["dlogits"] = run_bwd(ctx, guards, dl, dy, (n, h, w), f, outs)
        runs.append(got)
    for k in runs[0]:
        assert np.array_equal(bits(runs[0][k]), bits(runs[1][k])), k


# --------------------------------------------------------------------------------------------------- 9. standalone
@pytest.mark.parametrize("n,h,w,f", [(2, 12, 16, 4), (3, 5, 3, 8), (2, 3, 5, 1)])        # (x1: 15 pixels per image, the 4-byte read path)
def test_standalone_loss_agrees_with_the_fused_head(ctx, guards, n, h, w, f):
    logits, y, _, _, _, _ = head_case(n, h, w, f)
    hw = h * f * w * f
    keep = B.keep_count(0.25, hw)
    outs, got = run_fwd(ctx, guards, guards.inp(logits), guards.inp(y), (n, h, w), f, keep)
    alone = guards.out(n)
    ctx.call("ssdseg_bootstrap_ce_loss", guards.inp(y), outs["prob"], n, hw, 4, c4(CW32), keep, alone)
    ctx.sync()
    want = B.bootstrapped_cross_entropy(y, got["prob"], CW32, keep)[0]
    print("standalone vs fused", rel_err(alone.download(), got["loss"]), "vs oracle on the float32 probabilities", rel_err(alone.download(), want))
    assert rel_err(alone.download(), got["loss"]) < 1e-5
    assert rel_err(alone.download(), want) < 1e-5


# ------------------------------------------------------------------------------------------------------ engine-level tests
@pytest.fixture
def poison(ctx):
    """every activation, statistics table and workspace region of the engine starts as NaN (tests/_guard.py)"""
    ctx.debug_poison(True)
    try:
        yield ctx
    finally:
        ctx.debug_poison(False)


def compile_mask(model, mask_loss):
    import ssdseglib
    model.compile(optimizer=ssdseglib.optimizers.Adam(learning_rate=1e-4),
                  loss={'output-mask': mask_loss, 'output-labels': ssdseglib.losses.confidence_loss, 'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights={'output-mask': 1.0, 'output-labels': 1.0, 'output-boxes': 1.0})


def mask_op(eng):
    return next(op for _, op, kind in eng._loss_names if kind == "mask")


def engine_with_probabilities(model, batch, ctx):
    from ssdseglib import _engine as E
    E.Engine.keep_mask_probabilities = True         # (so that output(0) can be compared)
    try:
        eng = E.Engine(model, batch, training=True, ctx=ctx)
    finally:
        E.Engine.keep_mask_probabilities = False
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    return eng


# ------------------------------------------------------------------------------------------------- 10. whole-step parity
def test_full_train_step_parity_with_the_bootstrapped_mask_loss(ctx, poison, rng):
    """test_full_train_step_parity's set-up and bounds with output-mask compiled to bootstrapped_cross_entropy(CW, 0.25).  The
    oracle's mask loss and gradient take the keep mask downloaded from the op (pixel_loss >= thresh); that mask may differ from
    the oracle's own selection only near the threshold: the outputs agree within 2e-4 (asserted), so a pixel's loss is off by at
    most d_i = w_c (log p - log(p - 2e-4)) and the threshold -- an order statistic, 1-Lipschitz in the largest change -- by at
    most max d, and every differing pixel has |l_ref - tau_ref| <= 2 max d"""
    import ssdseglib
    batch = 3
    boxes, builder, model = build()
    for l in model.layers:
        if type(l).__name__ == "BatchNormalization":
            c = l.weights["gamma"].size
            l.weights["gamma"] = rng.uniform(0.7, 1.3, c).astype(np.float32)
            l.weights["beta"] = rng.normal(0, 0.3, c).astype(np.float32)
    enc, gts, targets = make_targets(rng, boxes, batch)
    assert targets['output-labels'][..., 1:].sum() > 0, "test needs at least one positive anchor"
    compile_mask(model, ssdseglib.losses.bootstrapped_cross_entropy(CW, 0.25))
    eng = engine_with_probabilities(model, batch, ctx)
    op = mask_op(eng)
    hw = SHAPE[0] * SHAPE[1]
    assert op.kind == "bootstrapped_cross_entropy" and op.keep == hw // 4 and op.pixel_loss.shape == (batch, hw)
    x = rng.integers(0, 256, (batch,) + SHAPE).astype(np.float32)

    ref = NpModel(model, dtype=np.float64)
    p_mask, p_labels, p_boxes = ref.forward(x, training=True)
    y_mask = targets['output-mask'].astype(np.float64)
    l_conf, dconf, _ = O.confidence_loss(targets['output-labels'].astype(np.float64), p_labels)
    l_loc, dloc = O.localization_loss(targets['output-boxes'].astype(np.float64), p_boxes)

    eng.set_input(x)
    eng.set_targets(targets)
    eng.forward()
    assert np.abs(eng.output(0) - p_mask).max() < 2e-4
    assert np.abs(eng.output(1) - p_labels).max() < 2e-4
    assert rel(eng.output(2), p_boxes) < 1e-3
    keep_dev = (op.pixel_loss.download() >= op.thresh.download()[:, None]).reshape(p_mask.shape[:-1])
    assert np.array_equal(op.kept.download(), keep_dev.reshape(batch, -1).sum(axis=1)) and (op.kept.download() >= op.keep).all()
    l_ref = B.pixel_losses(y_mask, p_mask, CW64)
    _, _, mask_ref, tau_ref = B.bootstrapped_cross_entropy(y_mask, p_mask, CW64, op.keep)
    p_true = np.clip((p_mask * y_mask).sum(axis=-1), 4e-4, None)
    d = ((y_mask * CW64).sum(axis=-1) * (np.log(p_true) - np.log(p_true - 2e-4))).max()
    differs = keep_dev != mask_ref
    print(f"keep mask differs from the oracle's own in {int(differs.sum())} of {differs.size} pixels, band 2 x {d:.3e}")
    assert (np.abs(l_ref - tau_ref[:, None, None])[differs] <= 2 * d).all()
    l_mask, dmask = B.with_keep_mask(y_mask, p_mask, CW64, keep_dev)

    got = eng.losses()
    assert abs(got['output-mask_loss'] - l_mask.mean()) < 1e-3 * abs(l_mask.mean())
    assert abs(got['output-labels_loss'] - l_conf.mean()) < 1e-3 * abs(l_conf.mean())
    assert abs(got['output-boxes_loss'] - l_loc.mean()) < 1e-3 * abs(l_loc.mean())
    assert abs(got['loss'] - (l_mask.mean() + l_conf.mean() + l_loc.mean())) < 1e-3 * got['loss']

    eng.backward()
    ctx.sync()
    ref_grads = ref.backward([dmask / batch, dconf / batch, dloc / batch], relu_masks=device_relu_masks(eng, model))
    worst, worst_name = 0.0, ""
    for l in model.layers:
        if not l.weights:
            continue
        scale = max(np.abs(ref_grads[l.name][w]).max() for w in l.trainable_names)
        if scale == 0:
            assert all(np.abs(eng.grad_view(l, w).download()).max() < 1e-12 for w in l.trainable_names), l.name
            continue
        for wname in l.trainable_names:
            g = eng.grad_view(l, wname).download()
            err = np.abs(g.astype(np.float64) - ref_grads[l.name][wname]).max() / scale
            if err > worst:
                worst, worst_name = err, f"{l.name}/{wname}"
            assert err < 1e-3, f"{l.name}/{wname}: rel err {err:.3e}"
    print("worst parameter-gradient rel err", worst, worst_name)


# ---------------------------------------------------------------------------------------------------------- 11. Keras surface
def test_bootstrapped_loss_through_compile_and_fit(ctx, poison, rng):
    """compile(loss={'output-mask': bootstrapped_cross_entropy(...)}) and two one-step fit calls on compact batches with compact
    validation_data: the history keys are the other mask losses', everything is finite, and the first step's `output-mask_loss` is
    the standalone callable's value on the engine's own targets and probabilities"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    boxes, _, model = build(seed=5)
    loss_fn = ssdseglib.losses.bootstrapped_cross_entropy(CW, 0.25)
    compile_mask(model, loss_fn)

    def compact(n):
        enc, gts, targets = make_targets(rng, boxes, n)
        img = rng.integers(0, 256, (n,) + SHAPE).astype(np.uint8)
        return ssdseglib.datacoder.CompactBatch(img, targets['output-mask'].argmax(-1).astype(np.uint8), gts, np.zeros(n, np.uint8), enc)

    train, val = compact(3), compact(2)
    keys = {'loss', 'output-mask_loss', 'output-labels_loss', 'output-boxes_loss'}
    E.Engine.keep_mask_probabilities = True
    try:
        for step in range(2):
            hist = model.fit([train], epochs=1, validation_data=[val], verbose=0).history
            assert set(hist) >= keys | {"val_" + k for k in keys}, sorted(hist)
            assert all(len(v) == 1 and np.isfinite(v[0]) for v in hist.values()), hist
            total = sum(hist[f"{k}_loss"][0] for k in ('output-mask', 'output-labels', 'output-boxes'))
            assert abs(hist['loss'][0] - total) <= 1e-6 * abs(total)
            if step == 0:
                eng = model._engines[(3, True)]
                op = mask_op(eng)
                assert op.kind == "bootstrapped_cross_entropy" and mask_op(model._engines[(2, "eval")]).kind == "bootstrapped_cross_entropy"
                assert op.keep == mask_op(model._engines[(2, "eval")]).keep == SHAPE[0] * SHAPE[1] // 4
                y, p = op.y_true.download(), eng.output(0)
                alone = loss_fn(y, p)
                assert alone.shape == (3,) and alone.dtype == np.float32
                assert abs(hist['output-mask_loss'][0] - alone.mean()) <= 1e-5 * abs(alone.mean())
                want = B.bootstrapped_cross_entropy(y, p.astype(np.float32), CW32, op.keep)[0]
                assert rel_err(alone, want) < 1e-5
    finally:
        E.Engine.keep_mask_probabilities = False


# --------------------------------------------------------------------------------------------------- 12. nothing else moves
def test_cross_entropy_step_touches_nothing_new(ctx, poison, rng, monkeypatch):
    import ssdseglib
    from ssdseglib import _engine as E
    batch = 3
    boxes, builder, model = build(seed=23)
    enc, gts, targets = make_targets(rng, boxes, batch)
    compile_mask(model, ssdseglib.losses.cross_entropy(classes_weights=CW))
    eng = E.Engine(model, batch, training=True, ctx=ctx)
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    op = mask_op(eng)
    assert op.kind == "cross_entropy" and op.pixel_loss is None and op.thresh is None and op.kept is None
    called = []
    real_call = ctx.call

    def spy(name, *args):
        called.append(name)
        return real_call(name, *args)

    eng.set_input(rng.integers(0, 256, (batch,) + SHAPE).astype(np.float32))
    eng.set_targets(targets)
    with monkeypatch.context() as m:
        m.setattr(ctx, "call", spy)
        eng.forward()
        eng.backward()
    ctx.sync()
    assert "ssdseg_mask_head_fwd" in called and "ssdseg_mask_head_bwd" in called
    assert not set(called) & set(NEW_ENTRIES)
