"""CPU: the BatchNorm partial-statistics table sizes of the depthwise conv (ssdseg_dwconv_parts), pinned.

The engine sizes each table once from this number; it is the larger block count of the two forward kernels that can take the
layer, i.e. the output of the geometry functions of csrc/dwconv.hip, csrc/dwconv_march.h and csrc/dwconv_lds.h at that shape.
The values were recorded from the library built at the commit named in RECORDED_FROM (the parent of the commit that put the
marching kernels' three geometry functions into one), never from the code under test."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ssdseglib import _hip
    if not os.path.exists(_hip.library_path()):
        g.build()
    return _hip.load_library()


RECORDED_FROM = "9d7ab19a2672a42359f91174fe1b9078f7d32e6a"
# (n, h, w, c, stride, dilation): rows -- the dw shapes of test_bn_partial_tables_do_not_depend_on_dispatch_switches, DW_CASES of
# tests/test_gpu_conv_ops.py, and two 64-channel chunks at both strides / one 144-channel chunk with w % 4 != 0
PARTS = {
    (2, 15, 20, 32, 1, 1): 8,
    (2, 15, 20, 32, 2, 1): 8,
    (1, 30, 40, 144, 2, 1): 24,
    (2, 8, 10, 960, 1, 1): 8,
    (1, 9, 7, 8, 2, 1): 8,
    (2, 12, 16, 64, 1, 6): 72,
    (32, 30, 40, 256, 1, 12): 4608,
    (32, 240, 320, 96, 2, 1): 2560,
    (32, 240, 320, 32, 1, 1): 1280,
    (32, 120, 160, 256, 1, 1): 512,
    (32, 120, 160, 144, 2, 1): 2560,
    (32, 30, 40, 576, 1, 1): 232,
    (3, 48, 64, 96, 2, 1): 96,
    (1, 10, 7, 8, 2, 1): 8,
    (1, 9, 8, 8, 2, 1): 8,
    (2, 30, 40, 64, 1, 3): 40,
    (1, 30, 40, 32, 1, 12): 144,
    (1, 30, 40, 576, 1, 6): 104,
    (2, 7, 5, 8, 1, 3): 24,
    (1, 4, 5, 8, 1, 12): 144,
    (1, 5, 6, 1284, 1, 1): 8,
    (1, 1, 1, 4, 1, 1): 8,
    (1, 12, 16, 128, 1, 1): 8,
    (1, 12, 16, 128, 2, 1): 8,
    (1, 12, 18, 144, 1, 1): 16,
}


@pytest.mark.parametrize("shape", list(PARTS))
def test_dwconv_parts_are_pinned(lib, shape):
    v = C.c_int()
    assert lib.ssdseg_dwconv_parts(*shape, C.byref(v)) == 0
    assert v.value == PARTS[shape]
