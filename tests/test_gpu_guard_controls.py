"""Controls of the guarded-buffer checks (tests/_guard.py): each check is shown to fail on a deliberately wrong call.  Every
wrong call here writes and reads only inside the test's own guarded allocations (the guards are 64 KiB and more, the errors one
row); none of them can fault."""
import numpy as np
import pytest

from oracle import np_ops as O
from _guard import BODY_WORD, Guards, assert_finite_rows, guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

M, K, N = 300, 24, 40


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _pw_case(rng):
    x = rng.normal(0, 1, (M, K)).astype(np.float32)
    wgt = (rng.normal(0, 1, (K, N)) / np.sqrt(K)).astype(np.float32)
    return x, wgt, x.astype(np.float64) @ wgt.astype(np.float64)


def test_control_unwritten_row_is_reported(ctx, guards, rng):
    from ssdseglib import _hip as H
    x, wgt, y_ref = _pw_case(rng)
    y = guards.out((M, N))
    ctx.call("ssdseg_pwconv_fwd", H.view(guards.inp(x)), K, guards.inp(wgt), y, N, M - 1, K, N, None)     # one row short
    idx = guards.unwritten(y)
    assert np.array_equal(idx, np.stack([np.full(N, M - 1), np.arange(N)], axis=1))
    with pytest.raises(AssertionError):
        assert rel_err(y.download(), y_ref) < 2e-5
    assert rel_err(y.download()[:-1], y_ref[:-1]) < 2e-5


def test_control_overrun_hits_the_back_guard(ctx, guards, rng):
    from ssdseglib import _hip as H
    x, wgt, y_ref = _pw_case(rng)
    g = Guards(ctx)          # its own guards: the fixture's teardown check must still pass
    y = g.out((M, N), name="y")
    shifted = ctx.borrow(y.ptr + N * 4, (M, N), owner=y)          # one row later: the last row lands in the back guard
    ctx.call("ssdseg_pwconv_fwd", H.view(guards.inp(x)), K, guards.inp(wgt), shifted, N, M, K, N, None)
    with pytest.raises(AssertionError, match=rf"y: back guard written at word offset 0 \({N} words\)"):
        g.check()
    assert guards.unwritten(y).shape[0] == N                       # the first row was skipped
    g.release()


def test_control_input_over_read_gives_nan(ctx, guards, rng):
    from ssdseglib import _hip as H
    x, wgt, y_ref = _pw_case(rng)
    dx = guards.inp(x)
    late = ctx.borrow(dx.ptr + K * 4, (M, K), owner=dx)            # its last row lies in the input's NaN guard
    y = guards.out((M, N))
    ctx.call("ssdseg_pwconv_fwd", H.view(late), K, guards.inp(wgt), y, N, M, K, N, None)
    got = y.download()
    assert np.isnan(got[-1]).all()
    assert np.isfinite(got[:-1]).all() and rel_err(got[:-1], y_ref[1:]) < 2e-5


def test_control_workspace_handouts_are_poisoned(ctx, guards, rng):
    """the BatchNorm partial table of ssdseg_channel_stats (a poisoned output) and the workspace partials of
    ssdseg_bn_bwd_reduce (a poisoned handout, counted) are written in full: the folded sums match the oracle"""
    m, c = 5000, 96
    y = rng.normal(0.5, 2.0, (m, c)).astype(np.float32)
    dy = guards.inp(y)
    nparts = ctx.parts("ssdseg_channel_stats_parts", m, c)
    st = guards.out((nparts, 2, c))
    ctx.call("ssdseg_channel_stats", dy, c, m, c, st)
    assert_finite_rows(st.download(), "channel stats")
    tot = st.download().astype(np.float64).sum(axis=0)
    assert rel_err(tot[0], y.sum(axis=0, dtype=np.float64)) < 1e-5
    assert rel_err(tot[1], (y.astype(np.float64) ** 2).sum(axis=0)) < 1e-5
    gamma = np.ones(c, np.float32)
    z_ref, cache = O.bn_train_fwd(y, gamma, np.zeros(c, np.float32))
    g = rng.normal(0, 1, (m, c)).astype(np.float32)
    _, dgamma_ref, dbeta_ref = O.bn_train_bwd(g, y, gamma, cache)
    coef = [guards.inp(cache[k].astype(np.float32)) for k in ("scale", "shift", "mean", "invstd")]
    outs = [guards.out(c) for _ in range(4)]
    before = ctx.debug_poison(True)
    ctx.call("ssdseg_bn_bwd_reduce", guards.inp(g), c, dy, c, m, c, *coef, O.ACT_NONE, *outs)
    after = ctx.debug_poison(True)
    assert after > before
    assert rel_err(outs[0].download(), dgamma_ref) < 1e-4
    assert rel_err(outs[1].download(), dbeta_ref) < 1e-4


def test_control_fresh_memory_is_poisoned(ctx, guards):
    got = ctx.empty((1000,), np.int32).download()
    assert (got.view(np.uint32) == BODY_WORD).all()
