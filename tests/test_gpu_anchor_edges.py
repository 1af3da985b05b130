"""GPU parity of the anchor-side kernels and of Adam at their edges (through the C-ABI) vs the NumPy oracle.

The cases come from tests/_anchor_cases.py; tests/test_cpu_anchor_edge_cases.py proves on the oracle alone that each case has
the property it is named for.  Index results (matches, labels, NMS rows, suppression) are bit-exact; encoded offsets hold a
float32 log and decoded corners a float32 exp: 1e-5 absolute / relative, as in tests/test_gpu_head_ops.py.
"""
import ctypes as C

import numpy as np
import pytest

import _anchor_cases as AC
from oracle import np_ops as O
from _guard import guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

STDS_C = (C.c_float * 4)(*AC.STDS)


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


# ---------------------------------------------------------------------------------------------------------------- encode
@pytest.mark.parametrize("name", list(AC.ENCODE_CASES))
def test_encode_targets_edges(ctx, guards, name):
    inputs, _ = AC.ENCODE_CASES[name]()
    anchors, gt, cnt, gmax, c, thr = (inputs[k] for k in ("anchors", "gt", "cnt", "gmax", "c", "thr"))
    a, b = anchors.shape[0], cnt.size
    d_anchors, d_gt, d_cnt = guards.inp(anchors), guards.inp(gt), guards.inp(cnt)
    labels, boxes, match = guards.out((b, a, c)), guards.out((b, a, 4)), guards.out((b, a), np.int32)
    ctx.call("ssdseg_encode_targets", d_anchors, a, d_gt, d_cnt, b, gmax, c, thr, STDS_C, labels, boxes, match)
    L, B, M = labels.download(), boxes.download(), match.download()
    for i in range(b):
        l_ref, b_ref, m_ref = AC.oracle_encode(inputs, i)      # a count beyond gmax: the oracle on the first gmax rows
        assert np.array_equal(M[i], m_ref), f"image {i}: {int((M[i] != m_ref).sum())} matched ground-truth indices differ"
        assert np.array_equal(L[i], l_ref), f"image {i}: labels differ"
        assert np.abs(B[i] - b_ref).max() < 1e-5, f"image {i}"
    if name.startswith("hand"):
        assert M[0].tolist() == AC.HAND_MATCH[thr] and (M[2] == -1).all()
    # the form every training step uses: no match output, the same labels and boxes bit for bit
    labels2, boxes2 = guards.out((b, a, c)), guards.out((b, a, 4))
    ctx.call("ssdseg_encode_targets", d_anchors, a, d_gt, d_cnt, b, gmax, c, thr, STDS_C, labels2, boxes2, None)
    assert np.array_equal(labels2.download(), L)
    assert np.array_equal(boxes2.download().view(np.uint32), B.view(np.uint32))
    ctx.sync()
    guards.check()


# ---------------------------------------------------------------------------------------------------------------- decode
def decode_on_device(ctx, guards, offsets, cent):
    b, a = offsets.shape[:2]
    corners = guards.out((b, a, 4))
    ctx.call("ssdseg_decode_boxes", guards.inp(offsets), guards.inp(cent), b, a, STDS_C, corners)
    return corners


def test_decode_saturated_offsets(ctx, guards):
    inputs, _ = AC.nms_saturated()
    off, cent = inputs["offsets"], inputs["centroids"]
    got = decode_on_device(ctx, guards, off, cent).download()
    ref = O.decode_to_corners_pred(off, cent, AC.STDS)
    assert rel_err(got, ref) < 1e-5
    # exp(0) - 1 is exactly 0 on both sides: a zero offset gives corners inverted by exactly one pixel
    zw, zh = off[..., 2] == 0, off[..., 3] == 0
    assert zw.mean() > 0.2 and zh.mean() > 0.2
    assert (got[..., 1][zw] > got[..., 3][zw]).all() and (got[..., 0][zh] > got[..., 2][zh]).all()
    assert np.array_equal(AC.inverted(got)[zw | zh], AC.inverted(ref)[zw | zh])


def test_decode_second_grid_pass(ctx, guards):
    """b * a = 1,228,800 boxes against 4096 x 256 = 1,048,576 threads: the grid-stride loop makes a second, partial pass"""
    b, a = 128, 9600
    assert b * a > AC.GRID
    rng = np.random.default_rng(5)
    off, cent = AC.relu6_offsets(rng, (b, a, 4)), AC.centroids_for(a)
    got = decode_on_device(ctx, guards, off, cent).download()
    ref = O.decode_to_corners_pred(off, cent, AC.STDS)
    assert rel_err(got, ref) < 1e-5
    assert rel_err(got[-1, -256:], ref[-1, -256:]) < 1e-5      # the last boxes of the second pass
    ctx.sync()
    guards.check()


# ------------------------------------------------------------------------------------------------------------------- NMS
def run_nms(ctx, guards, inputs, with_valid=True):
    """-> (out, valid or None, the corners both sides use)"""
    if "corners" in inputs:
        d_corners = guards.inp(inputs["corners"])
    else:
        d_corners = decode_on_device(ctx, guards, inputs["offsets"], inputs["centroids"])
    cr = d_corners.download()
    probs = inputs["probs"]
    b, a, c = probs.shape
    out = guards.out((b, inputs["max_total"], 6))
    valid = guards.out(b, np.int32) if with_valid else None
    ctx.call("ssdseg_combined_nms", d_corners, guards.inp(probs), b, a, c, inputs["max_per_class"], inputs["max_total"], inputs["iou_thr"],
             inputs["score_thr"], out, valid)
    return out.download(), (valid.download() if with_valid else None), cr


@pytest.mark.parametrize("name", list(AC.NMS_CASES))
def test_combined_nms_edges(ctx, guards, name):
    inputs, _ = AC.NMS_CASES[name]()
    out, valid, cr = run_nms(ctx, guards, inputs)
    if "offsets" in inputs:
        assert rel_err(cr, AC.oracle_corners(inputs)) < 1e-5
    ref_out, ref_valid = AC.oracle_nms(inputs, cr)             # the same decoded boxes on both sides
    assert np.array_equal(valid, ref_valid)
    diff = np.argwhere((out != ref_out).any(-1))
    assert np.array_equal(out, ref_out), f"{len(diff)} rows differ, first (image, row) = {diff[0].tolist() if len(diff) else None}"
    for i in range(out.shape[0]):
        assert not out[i, valid[i]:].any()                       # the tail is zero-filled
    ctx.sync()
    guards.check()


def test_combined_nms_without_valid(ctx, guards):
    inputs, _ = AC.nms_saturated()
    out, _, cr = run_nms(ctx, guards, inputs, with_valid=False)
    assert np.array_equal(out, AC.oracle_nms(inputs, cr)[0])


# --------------------------------------------------------------------------------------------------- segmentation suppression
@pytest.mark.parametrize("name", AC.SEG_CASES)
def test_seg_suppress_edges(ctx, guards, name):
    inputs, _ = AC.seg_case(name)
    mask, probs = inputs["mask"], inputs["probs"]
    npix, rows = mask.shape[0] * mask.shape[1], probs.shape[0]
    out = guards.out((rows, 4))
    ctx.call("ssdseg_seg_suppress", guards.inp(mask), npix, 4, guards.inp(probs), rows, out)
    got = out.download()
    assert np.array_equal(got, O.seg_suppress(mask, probs))
    assert [bool(got[:, k].any()) for k in range(4)] == [bool(p) for p in AC.SEG_PRESENT[name]]
    ctx.sync()
    guards.check()


# ---------------------------------------------------------------------------------------------------------------------- Adam
ADAM_RUNS = [(n, 1, 50, s) for n in AC.ADAM_COUNTS[:-1] for s in (1.0, 0.125)] + \
            [(AC.ADAM_BIG, first, 3, s) for first in (1, 10000) for s in (1.0, 0.125)]


@pytest.mark.parametrize("count,first_step,steps,grad_scale", ADAM_RUNS)
def test_adam_step_vs_float64(ctx, guards, count, first_step, steps, grad_scale):
    """ssdseg_adam_step over consecutive steps against O.adam_step in float64 on the same float32 inputs (lr, beta, eps as the
    floats the C-ABI receives).  Bound: e32 = the largest difference, over parameters and both moments, between O.adam_step run in
    float32 and in float64; every output of the kernel is within 4 * e32 of the float64 result (the factor: the kernel rounds
    1 - beta and alpha to float once, NumPy promotes them).  From 1031 elements on, where the maximum over the elements is a
    stable estimate of each array's own rounding error, each array is also held to 4 * its own e32 (the moments are smaller
    numbers than the parameters, so this is the tighter bound for them); below that, the float32 error of a handful of elements
    can be zero by chance.

    Measured on an MI355X, largest error against float64 as e32 / kernel (run with -s for the current figures):
      count     first  scale   p                      m                      v
      1         1      1       5.22e-08 / 5.22e-08    3.87e-09 / 3.87e-09    8.19e-10 / 6.63e-09
      1         1      1/8     4.69e-08 / 1.71e-08    4.47e-10 / 4.47e-10    1.36e-10 / 1.36e-10
      3         1      1       1.88e-07 / 1.88e-07    6.89e-08 / 6.89e-08    1.99e-08 / 1.99e-08
      3         1      1/8     4.23e-07 / 4.23e-07    1.01e-08 / 1.01e-08    2.58e-10 / 1.95e-10
      4         1      1       3.14e-07 / 3.14e-07    6.71e-08 / 2.33e-08    1.28e-08 / 1.28e-08
      4         1      1/8     1.27e-07 / 1.27e-07    3.53e-09 / 6.66e-09    3.27e-10 / 3.26e-10
      5         1      1       8.08e-08 / 8.08e-08    3.39e-08 / 4.93e-08    1.65e-08 / 1.65e-08
      5         1      1/8     2.75e-07 / 2.75e-07    4.77e-09 / 4.77e-09    9.33e-10 / 9.33e-10
      1031      1      1       1.46e-06 / 1.46e-06    2.00e-07 / 1.27e-07    1.48e-07 / 1.18e-07
      1031      1      1/8     1.34e-06 / 1.34e-06    1.47e-08 / 2.14e-08    2.35e-09 / 2.35e-09
      2097158   1      1       6.12e-07 / 6.12e-07    2.03e-07 / 1.78e-07    2.72e-08 / 1.97e-08
      2097158   1      1/8     6.25e-07 / 6.25e-07    2.58e-08 / 2.14e-08    4.67e-10 / 3.89e-10
      2097158   10000  1       1.28e-06 / 6.31e-07    2.03e-07 / 1.78e-07    2.72e-08 / 1.97e-08
      2097158   10000  1/8     1.13e-06 / 7.77e-07    2.58e-08 / 2.14e-08    4.67e-10 / 3.89e-10
    The one-element case shows why the per-array bound starts at 1031: its v is 8 x its own e32 (8.19e-10, a lucky float32
    run) and a tenth of the case's e32."""
    inputs, _ = AC.adam_case(count, steps)
    h = AC.ADAM_HYPER
    ref64 = AC.adam_oracle(inputs, first_step, grad_scale, np.float64)
    ref32 = AC.adam_oracle(inputs, first_step, grad_scale, np.float32)
    e32 = [float(np.abs(r32.astype(np.float64) - r64).max()) for r32, r64 in zip(ref32, ref64)]
    p, m, v, g = (guards.out((count, 1)) for _ in range(4))       # one element per row: the back guard scales with the row pitch
    p.upload(inputs["p"]); m.upload(inputs["m"]); v.upload(inputs["v"])
    for s in range(steps):
        g.upload(inputs["g"][s])
        ctx.call("ssdseg_adam_step", p, g, m, v, C.c_size_t(count), h["lr"], h["b1"], h["b2"], h["eps"], first_step + s, grad_scale)
    ctx.sync()
    guards.check()                                               # count % 4 != 0: nothing beyond the last element is touched
    assert np.array_equal(g.download().ravel(), inputs["g"][-1])         # the gradient is read only
    err = [float(np.abs(buf.download().ravel().astype(np.float64) - r64).max()) for buf, r64 in zip((p, m, v), ref64)]
    moved = float(np.abs(ref64[0] - inputs["p"]).max())
    print(f"\nadam count={count} first_step={first_step} steps={steps} grad_scale={grad_scale}: moved {moved:.3g}; "
          + "; ".join(f"{n}: e32 {e:.3g} kernel {k:.3g}" for n, e, k in zip("pmv", e32, err)))
    case_e32 = max(e32)
    assert moved > 1000 * case_e32, "the movement does not dwarf the rounding"
    for name, k in zip("pmv", err):
        assert k <= 4 * case_e32, f"{name}: kernel error {k:.3g} against e32 {case_e32:.3g}"
    if count >= 1031:
        for name, k, e in zip("pmv", err, e32):
            assert k <= 4 * e, f"{name}: kernel error {k:.3g} against that array's e32 {e:.3g}"
