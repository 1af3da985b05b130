"""The focal confidence loss without a GPU: the public factory's surface, and the fp64 oracle (tests/_focal_oracle.py) pinned three
ways -- its gamma = 0, alpha = 1 limit is the un-mined cross-entropy, its analytic gradient agrees with central differences, and
value and gradient agree with the same loss written in torch (CPU autograd, float64).  test_gpu_focal_loss.py then pins the
kernel to the oracle."""
import numpy as np
import pytest

from oracle import np_ops as O
import _focal_oracle as F

ALPHAS = [(1.0, 1.0, 1.0, 1.0), (0.25, 1.0, 0.75, 0.5)]


def make_case(rng, b=2, a=12, pos_frac=0.4):
    """float64 probabilities well inside the clip range (softmax of logits in [0, 3]: every p in [0.016, 0.87]), one-hot targets"""
    p = O.softmax(rng.uniform(0, 3, (b, a, 4)))
    cls = np.where(rng.uniform(size=(b, a)) < pos_frac, rng.integers(1, 4, (b, a)), 0)
    assert p.min() > O.EPS + 1e-3 and p.max() < 1 - O.EPS - 1e-3
    return np.eye(4)[cls], p


def rel_err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# -------------------------------------------------------------------------------------------------------------- the surface
def test_factory_surface():
    import ssdseglib
    fn = ssdseglib.losses.focal_confidence_loss()
    assert fn.__name__ == "focal_confidence_loss" and fn.loss_kind == "focal"
    assert fn.alpha == (1.0, 1.0, 1.0, 1.0) and fn.gamma == 2.0
    fn = ssdseglib.losses.focal_confidence_loss(alpha=[0.25, 1, 0.75, 0.5], gamma=0)
    assert fn.alpha == (0.25, 1.0, 0.75, 0.5) and fn.gamma == 0.0 and callable(fn)
    assert all(type(w) is float for w in fn.alpha) and type(fn.gamma) is float


@pytest.mark.parametrize("kwargs", [dict(gamma=-0.5), dict(gamma=float("nan")), dict(alpha=(1.0, 1.0, 1.0)), dict(alpha=(1.0,) * 5),
                                    dict(alpha=(1.0, -0.1, 1.0, 1.0)), dict(alpha=(1.0, float("inf"), 1.0, 1.0)),
                                    dict(alpha=(1.0, float("nan"), 1.0, 1.0)), dict(alpha=1.0)])
def test_factory_rejects_bad_arguments_without_a_device(kwargs, monkeypatch):
    import ssdseglib
    from ssdseglib import _engine

    def no_device():
        raise AssertionError("the factory touched the GPU")
    monkeypatch.setattr(_engine, "default_context", no_device)
    with pytest.raises(ValueError):
        ssdseglib.losses.focal_confidence_loss(**kwargs)
    ssdseglib.losses.focal_confidence_loss((0.0, 1.0, 2.0, 3.0), 0.0)          # the edges of the valid range are accepted


# ------------------------------------------------------------------------------------------------------------- the oracle
def test_gamma_zero_alpha_one_is_the_unmined_cross_entropy():
    rng = np.random.default_rng(7)
    y, p = make_case(rng, b=3, a=40, pos_frac=0.1)
    y[2] = np.eye(4)[0]                                     # an image without objects: divide by 1
    npos = np.maximum((y[..., 0] == 0).sum(-1), 1)
    assert npos[2] == 1 and npos[0] > 1
    loss, dp = F.focal_confidence_loss(y, p, (1, 1, 1, 1), 0.0)
    want = -(y * np.log(np.clip(p, O.EPS, 1 - O.EPS))).sum(axis=(1, 2)) / npos
    assert np.abs(loss - want).max() <= 1e-14 * np.abs(want).max()
    dwant = -(y / np.clip(p, O.EPS, 1 - O.EPS)) / npos[:, None, None]
    assert np.array_equal(dp, dwant)                        # the gamma term is exactly zero, (1 - p)^0 exactly one


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("gamma", [0.5, 2.0, 5.0])
def test_gradient_against_central_differences(alpha, gamma):
    """h = 1e-6 on p >= 0.016: truncation h^2 f''' / 6 < 1e-7 absolute against gradients of order 1 .. 60, rounding
    1e-16 * |loss| / h ~ 1e-9: inside the 1e-6 relative bound"""
    rng = np.random.default_rng(11)
    y, p = make_case(rng)
    _, dp = F.focal_confidence_loss(y, p, alpha, gamma)
    h = 1e-6
    fd = np.zeros_like(dp)
    for idx in np.ndindex(*p.shape):
        up, dn = p.copy(), p.copy()
        up[idx] += h
        dn[idx] -= h
        lu, _ = F.focal_confidence_loss(y, up, alpha, gamma)
        ld, _ = F.focal_confidence_loss(y, dn, alpha, gamma)
        fd[idx] = (lu[idx[0]] - ld[idx[0]]) / (2 * h)
        other = [i for i in range(p.shape[0]) if i != idx[0]]
        assert np.array_equal(lu[other], ld[other])         # no image depends on another one
    assert np.abs(dp).max() > 1
    assert rel_err(dp, fd) < 1e-6
    assert not dp[y == 0].any() and not fd[y == 0].any()


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0, 5.0])
def test_value_and_gradient_against_torch_autograd(alpha, gamma):
    import torch
    rng = np.random.default_rng(13)
    y, p = make_case(rng, b=3, a=30, pos_frac=0.2)
    y[1] = np.eye(4)[0]
    loss, dp = F.focal_confidence_loss(y, p, alpha, gamma)
    ty = torch.tensor(y, dtype=torch.float64)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    ta = torch.tensor(alpha, dtype=torch.float64)
    ph = torch.clamp(tp, O.EPS, 1 - O.EPS)
    fl = -(ta * ty * (1 - ph) ** gamma * torch.log(ph)).sum(-1)
    tl = fl.sum(-1) / torch.clamp((ty[..., 0] - 1).abs().sum(-1), min=1.0)
    tl.sum().backward()
    assert rel_err(loss, tl.detach().numpy()) < 1e-12
    assert rel_err(dp, tp.grad.numpy()) < 1e-12


def test_clip_constants_follow_the_dtype_of_p():
    """float32 probabilities are clipped at the device's float32 constants, so 1 - clip(p) >= 2^-23 and nothing divides by zero"""
    p = np.array([[[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]]], np.float32)
    y = np.eye(4)[[[0, 0]]]
    ph, inside = F.clip_and_inside(p)
    assert ph.max() == 1 - 2.0 ** -23 and ph.min() == float(np.float32(1e-7)) and not inside.any()
    for gamma in (0.0, 0.5, 2.0, 5.0):
        loss, dp = F.focal_confidence_loss(y, p, (1, 1, 1, 1), gamma)
        assert np.isfinite(loss).all() and not dp.any()
