"""What the GPU edge suites (tests/test_gpu_tail_edges.py, tests/test_gpu_mask_edges.py, tests/test_gpu_dw_edges.py, tests/test_gpu_pw_edges.py,
tests/test_gpu_conv3_edges.py, tests/test_gpu_stem_edges.py) share: the error / bound ratio and its report,
the launches of a call read from the timing registry, bit comparisons, poison counts, views of guarded inputs, rejected calls."""
import ctypes as C

import numpy as np
import pytest

from oracle import np_ops as O
from _guard import BODY_WORD


def c4(values):
    return (C.c_float * 4)(*values)


def reporter(prefix):
    """-> report(kernel, case, **ratios), which prints (under `prefix`) and asserts the error / bound ratios of one case"""
    def report(kernel, case, **ratios):
        print(f"\n{prefix} {kernel} {case}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
        for k, v in ratios.items():
            assert v <= 1.0, f"{kernel} {case}: {k} is {v:.3g} x its bound"
    return report


def ratio(got, ref, bound):
    """largest |got - ref| / bound; where the bound is 0 the result must be exact"""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    bound = np.broadcast_to(bound, got.shape)
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} elements are not finite"
    err = np.abs(got - ref)
    exact = bound == 0
    assert not err[exact].any(), "an element whose bound is 0 differs"
    return float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0


def finish(ctx, guards):
    ctx.sync()
    guards.check()


def launched(ctx, fn):
    """{kernel symbol: launches} of the calls fn() makes"""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        fn()
        ctx.join()
        return {k: r["count"] for k, r in ctx.timing_report().items()}
    finally:
        ctx.timing(False)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def untouched(buf):
    """number of elements of an output body that still hold the poison"""
    return int((buf.download().view(np.uint32) == np.uint32(BODY_WORD)).sum())


def dev_view(guards, x, scale=None, shift=None, act=O.ACT_NONE, ld=None):
    from ssdseglib import _hip as H
    xb = guards.inp(x, ld=ld)
    if scale is None:
        return H.view(xb, act=act)
    return H.view(xb, guards.inp(scale), guards.inp(shift), act)


def rejected(ctx, name, *args):
    from ssdseglib import _hip as H
    with pytest.raises(H.SsdsegError, match=f"{name}: invalid argument"):
        ctx.call(name, *args)
