"""The bootstrapped cross-entropy (hard-pixel mining of the mask head) without a GPU: the public factory's surface and keep
formula, and the fp64 oracle (tests/_bootstrap_oracle.py) pinned four ways -- with every pixel kept it is
oracle.np_ops.cross_entropy_loss exactly, a hand-worked image, the tie rule, and central differences of its gradient.
test_gpu_mask_bootstrap.py then pins the kernels to the oracle."""
import math

import numpy as np
import pytest

from oracle import np_ops as O
import _bootstrap_oracle as B

CW = (0.05, 0.575, 0.135, 0.24)
LN2 = math.log(2.0)


def make_case(rng, n=2, h=5, w=7):
    """float64 probabilities well inside the clip range, one-hot targets"""
    p = O.softmax(rng.uniform(0, 3, (n, h, w, 4)))
    assert p.min() > O.EPS + 1e-3 and p.max() < 1 - O.EPS - 1e-3
    return np.eye(4)[rng.integers(0, 4, (n, h, w))], p


def hand_image():
    """1 x 2 x 3 pixels, weights (1, 2, 0.5, 0): classes 0 1 2 3 0 1 with true-class probabilities 1/2 1/2 1/4 1/10 1/8 1/4, so that
    l = (1, 2, 1, 0, 3, 4) ln 2 -- every product and the tie between pixels 0 and 2 exact in binary floating point"""
    cls = np.array([0, 1, 2, 3, 0, 1])
    q = np.array([0.5, 0.5, 0.25, 0.1, 0.125, 0.25])
    y = np.eye(4)[cls]
    p = np.where(y == 1, q[:, None], ((1 - q) / 3)[:, None])
    return y.reshape(1, 2, 3, 4), p.reshape(1, 2, 3, 4), (1.0, 2.0, 0.5, 0.0)


# -------------------------------------------------------------------------------------------------------------- the surface
def test_factory_surface():
    import ssdseglib
    fn = ssdseglib.losses.bootstrapped_cross_entropy(CW)
    assert fn.loss_kind == "bootstrapped_cross_entropy" and callable(fn)
    assert fn.classes_weights == CW and fn.keep_fraction == 0.25
    fn = ssdseglib.losses.bootstrapped_cross_entropy([1, 0, 2, 3], keep_fraction=1)
    assert fn.classes_weights == (1.0, 0.0, 2.0, 3.0) and fn.keep_fraction == 1.0
    assert all(type(w) is float for w in fn.classes_weights) and type(fn.keep_fraction) is float


@pytest.mark.parametrize("args", [((1.0, 1.0, 1.0), 0.25), ((1.0,) * 5, 0.25), (1.0, 0.25), ((1.0, -0.1, 1.0, 1.0), 0.25),
                                  ((1.0, float("inf"), 1.0, 1.0), 0.25), ((1.0, float("nan"), 1.0, 1.0), 0.25), (CW, 0.0), (CW, -0.25),
                                  (CW, 1.0000001), (CW, float("nan")), (CW, float("inf")), (CW, None)])
def test_factory_rejects_bad_arguments_without_a_device(args, monkeypatch):
    import ssdseglib
    from ssdseglib import _engine

    def no_device():
        raise AssertionError("the factory touched the GPU")
    monkeypatch.setattr(_engine, "default_context", no_device)
    with pytest.raises(ValueError):
        ssdseglib.losses.bootstrapped_cross_entropy(*args)
    ssdseglib.losses.bootstrapped_cross_entropy((0.0, 0.0, 0.0, 0.0), 1.0)          # the edges of the valid range are accepted
    ssdseglib.losses.bootstrapped_cross_entropy(CW, 5e-324)


def test_keep_formula_on_and_next_to_integers():
    """keep = min(H W, max(1, ceil(keep_fraction H W))) in double: fractions whose product with the pixel count is an integer, and
    their two neighbouring doubles"""
    import ssdseglib
    for keep in (ssdseglib.losses.bootstrap_keep, B.keep_count):
        assert keep(0.25, 1000) == 250
        assert keep(np.nextafter(0.25, 1.0), 1000) == 251
        assert keep(np.nextafter(0.25, 0.0), 1000) == 250
        assert keep(0.5, 480 * 640) == 153600 and keep(np.nextafter(0.5, 1.0), 480 * 640) == 153601
        assert keep(0.125, 15) == 2                                               # 1.875
        assert keep(0.07, 100) == 8                                               # the double product as it stands: 7.000000000000001
        assert keep(1.0, 77) == 77 and keep(np.nextafter(1.0, 0.0), 77) == 77
        assert keep(1e-9, 77) == 1 and keep(5e-324, 480 * 640) == 1 and keep(1.0 / 77, 77) == 1
        assert keep(0.03, 48 * 64) == math.ceil(0.03 * 3072) == 93


# ------------------------------------------------------------------------------------------------------------- the oracle
def test_keeping_every_pixel_is_the_cross_entropy_exactly():
    y, p = make_case(np.random.default_rng(3))
    w = np.asarray(CW)
    loss, dp, mask, thresh = B.bootstrapped_cross_entropy(y, p, w, 35)
    want, dwant = O.cross_entropy_loss(y, p, w)
    assert mask.all() and np.array_equal(loss, want) and np.array_equal(dp, dwant)
    assert np.array_equal(thresh, B.pixel_losses(y, p, w).reshape(2, -1).min(axis=1))
    assert np.abs(B.pixel_losses(y, p, w).reshape(2, -1).sum(axis=1) - want).max() < 1e-12 * want.max()


def test_hand_worked_image():
    y, p, w = hand_image()
    l = B.pixel_losses(y, p, w)
    assert np.array_equal(l.ravel(), np.array([1, 2, 1, 0, 3, 4]) * LN2)
    loss, dp, mask, thresh = B.bootstrapped_cross_entropy(y, p, w, 2)
    assert thresh[0] == 3 * LN2 and mask.ravel().tolist() == [False, False, False, False, True, True]
    assert abs(loss[0] - 7 * LN2) < 1e-15
    want = np.zeros((6, 4))
    want[4, 0], want[5, 1] = -1.0 / 0.125, -2.0 / 0.25
    assert np.array_equal(dp.reshape(6, 4), want)
    loss, dp, mask, thresh = B.bootstrapped_cross_entropy(y, p, w, 3)
    assert thresh[0] == 2 * LN2 and mask.sum() == 3 and abs(loss[0] - 9 * LN2) < 1e-15
    assert dp.reshape(6, 4)[1, 1] == -2.0 / 0.5 and not dp.reshape(6, 4)[[0, 2, 3]].any()
    # keep = 1 and keep = H W
    loss, _, mask, thresh = B.bootstrapped_cross_entropy(y, p, w, 1)
    assert thresh[0] == 4 * LN2 and mask.sum() == 1 and loss[0] == 4 * LN2
    loss, dp, mask, thresh = B.bootstrapped_cross_entropy(y, p, w, 6)
    assert thresh[0] == 0 and mask.all() and abs(loss[0] - 11 * LN2) < 1e-15
    assert not dp.reshape(6, 4)[3].any()                                            # the weight-0 class: kept, and no gradient


def test_every_pixel_tied_with_the_kth_value_is_kept():
    y, p, w = hand_image()
    # keep = 4 falls on the tie between pixels 0 and 2 (l = ln 2 both): both are kept, five pixels count
    loss, dp, mask, thresh = B.bootstrapped_cross_entropy(y, p, w, 4)
    assert thresh[0] == LN2 and mask.sum() == 5 > 4 and mask.ravel().tolist() == [True, True, True, False, True, True]
    assert abs(loss[0] - 11 * LN2) < 1e-15
    assert dp.reshape(6, 4)[0, 0] == -1.0 / 0.5 and dp.reshape(6, 4)[2, 2] == -0.5 / 0.25
    same = B.bootstrapped_cross_entropy(y, p, w, 5)
    assert np.array_equal(same[2], mask) and same[0][0] == loss[0] and same[3][0] == thresh[0]
    # a given mask: the tie broken by hand
    mask4 = mask.copy()
    mask4[0, 0, 2] = False
    loss4, dp4 = B.with_keep_mask(y, p, w, mask4)
    assert abs(loss4[0] - 10 * LN2) < 1e-15 and not dp4[0, 0, 2].any() and np.array_equal(dp4[0, 0, :2], dp[0, 0, :2])


def test_gradient_against_central_differences():
    rng = np.random.default_rng(11)
    y, p = make_case(rng, n=2, h=3, w=4)
    w = np.asarray(CW)
    keep = 5
    l = np.sort(B.pixel_losses(y, p, w).reshape(2, -1), axis=1)[:, ::-1]
    gap = (l[:, keep - 1] - l[:, keep]).min()
    assert gap > 1e-3, "the case needs its keep-th and (keep+1)-th losses apart"
    loss, dp, mask, _ = B.bootstrapped_cross_entropy(y, p, w, keep)
    assert (mask.reshape(2, -1).sum(axis=1) == keep).all()
    h = 1e-6                                                # moves l by at most w / p * h < 4e-5, far below the gap: the selection stays put
    num = np.zeros_like(dp)
    for idx in np.ndindex(p.shape):
        hi, lo = p.copy(), p.copy()
        hi[idx] += h
        lo[idx] -= h
        num[idx] = (B.bootstrapped_cross_entropy(y, hi, w, keep)[0][idx[0]] - B.bootstrapped_cross_entropy(y, lo, w, keep)[0][idx[0]]) / (2 * h)
    assert np.abs(num - dp).max() < 1e-6 * np.abs(dp).max()
    assert not dp[~mask].any() and (dp[mask] != 0).any(axis=-1).all()
