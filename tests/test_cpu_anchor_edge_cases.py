"""Every case of tests/_anchor_cases.py has the property it is named for (CPU only, oracle only).

The GPU file runs the kernels on these cases and compares with the oracle; this file proves that the cases reach the edges: the
oracle's own answer changes when the edge is removed (no min/max swap, a threshold one float32 lower, a limit one larger).  These
are conditions on the inputs, not measurements of the code under test.
"""
import numpy as np
import pytest

import _anchor_cases as AC
from oracle import np_ops as O

F32 = np.float32


def rows_of(out, valid, image=0):
    return [tuple(r) for r in out[image, :valid[image]]]


# ------------------------------------------------------------------------------------------------------------------- NMS
def test_saturated_case_decodes_inverted_boxes_that_decide_the_selection(monkeypatch):
    inputs, _ = AC.nms_saturated()
    off = inputs["offsets"]
    assert (off == 0).mean() >= 0.20 and (off == 6).mean() >= 0.02
    corners = AC.oracle_corners(inputs)
    inv = AC.inverted(corners)
    assert inv.mean() >= 0.25
    out, valid = AC.oracle_nms(inputs, corners)
    assert (valid == inputs["max_total"]).all()
    picked_inverted = sum(int(r[2] > r[4] or r[3] > r[5]) for i in range(out.shape[0]) for r in rows_of(out, valid, i))
    assert picked_inverted >= 1, "no inverted box among the selected detections"
    # a candidate is suppressed by a kept box: without suppression (IoU never exceeds 1) the selection differs
    out_all, _ = AC.oracle_nms(inputs, corners, iou_thr=1.0)
    assert not np.array_equal(out, out_all)

    # the min/max swap decides: an IoU that takes the corners as given (negative extents -> area <= 0 -> 0) selects other boxes
    def iou_no_swap(a, b):
        area_a, area_b = F32(a[2] - a[0]) * F32(a[3] - a[1]), F32(b[2] - b[0]) * F32(b[3] - b[1])
        if area_a <= 0 or area_b <= 0:
            return F32(0)
        inter = F32(max(F32(min(a[2], b[2]) - max(a[0], b[0])), F32(0))) * F32(max(F32(min(a[3], b[3]) - max(a[1], b[1])), F32(0)))
        return F32(inter / F32(F32(area_a + area_b) - inter))
    monkeypatch.setattr(O, "_iou_tf", iou_no_swap)
    out_ns, _ = AC.oracle_nms(inputs, corners)
    assert not np.array_equal(out, out_ns), "the selection does not depend on the swap of inverted corners"


def test_tied_case_has_ties_across_both_limits():
    inputs, _ = AC.nms_tied()
    assert np.array_equal(inputs["probs"] * 16, np.round(inputs["probs"] * 16))
    corners = AC.oracle_corners(inputs)
    out, valid = AC.oracle_nms(inputs, corners)
    mt, mpc, c = inputs["max_total"], inputs["max_per_class"], inputs["c"]
    rows = rows_of(out, valid)
    scores = [r[1] for r in rows]
    boxes = [r[2:] for r in rows]
    assert any(scores[i] == scores[j] and boxes[i] != boxes[j] for i in range(len(rows)) for j in range(i)), "no equal scores at different anchors"
    # an equal-score pair straddles the max_total cut: rows max_total - 1 and max_total of the uncut merge
    full, fvalid = AC.oracle_nms(inputs, corners, max_total=c * mpc)
    assert fvalid[0] > mt and full[0, mt - 1, 1] == full[0, mt, 1]
    assert np.array_equal(full[0, :mt], out[0])
    # ... and a max_per_class cut: with one more per class, the extra pick of some class has the score of that class's last pick
    more, mvalid = AC.oracle_nms(inputs, corners, max_per_class=mpc + 1, max_total=c * (mpc + 1))
    straddles = 0
    for cl in range(c):
        s = sorted((r[1] for r in rows_of(more, mvalid) if r[0] == cl), reverse=True)
        straddles += len(s) == mpc + 1 and s[mpc - 1] == s[mpc]
    assert straddles >= 1


def test_exact_iou_threshold_changes_the_selection_by_one_box_per_pair():
    on, _ = AC.nms_exact_iou_threshold(0.5)
    below, _ = AC.nms_exact_iou_threshold(AC.HALF_BELOW)
    c = on["corners"][0]
    assert O._iou_tf(c[0], c[1]) == F32(0.5) and O._iou_tf(c[3], c[4]) == F32(0.5)
    (o1, v1), (o2, v2) = AC.oracle_nms(on), AC.oracle_nms(below)
    keep1 = {r[2:] for r in rows_of(o1, v1) if r[0] == 1}
    keep2 = {r[2:] for r in rows_of(o2, v2) if r[0] == 1}
    assert len(keep1) == 5 and keep2 < keep1 and len(keep1 - keep2) == 2      # the lower-scoring box of each pair goes


def test_exact_score_threshold_changes_the_selection_by_one_box():
    on, _ = AC.nms_exact_score_threshold(AC.SCORE_06)
    below, _ = AC.nms_exact_score_threshold(AC.SCORE_06_BELOW)
    (o1, v1), (o2, v2) = AC.oracle_nms(on), AC.oracle_nms(below)
    assert v1[0] == 2 and v2[0] == 4                      # class 1: + the box at 0.6; class 0: + the box at 0.6
    assert all(r[1] > F32(0.6) for r in rows_of(o1, v1))
    assert sorted(r[1] for r in rows_of(o2, v2))[:2] == [F32(0.6), F32(0.6)]
    assert F32(AC.SCORE_06_BELOW) not in [r[1] for r in rows_of(o2, v2)]      # a score equal to the lower threshold stays out


def test_thread_tie_case_picks_the_lowest_anchor():
    inputs, _ = AC.nms_thread_ties()
    out, valid = AC.oracle_nms(inputs)
    cr = inputs["corners"]
    want = {0: {1: 5, 2: 700, 3: 31}, 1: {1: 1023, 2: 1023, 3: 1}}
    for img in (0, 1):
        got = {int(r[0]): r[2:] for r in rows_of(out, valid, img)}
        assert set(got) == {1, 2, 3}
        for cl, anchor in want[img].items():
            y0, x0, y1, x1 = cr[img, anchor]
            assert got[cl] == (x0, y0, x1, y1), (img, cl)
        assert len({r[1] for r in rows_of(out, valid, img)}) == 1            # one score: the merge orders by anchor, then class


def test_dry_case_runs_every_class_dry():
    inputs, _ = AC.nms_dry()
    out, valid = AC.oracle_nms(inputs)
    for img in range(out.shape[0]):
        per_class = np.bincount(out[img, :valid[img], 0].astype(int), minlength=inputs["c"])
        assert (per_class >= 1).all() and (per_class < inputs["max_per_class"]).all()
        assert valid[img] < inputs["max_total"] and not out[img, valid[img]:].any()
    assert inputs["max_total"] > inputs["c"] * inputs["max_per_class"]


@pytest.mark.parametrize("a,c,mpc,mt", AC.NMS_GEOMETRIES)
def test_geometry_cases(a, c, mpc, mt):
    inputs, _ = AC.nms_geometry(a, c, mpc, mt)
    assert inputs["probs"].shape == (2, a, c)
    out, valid = AC.oracle_nms(inputs)
    assert valid[0] >= 1 and valid[1] == 0 and not out[1].any()
    assert (inputs["probs"][1] == F32(inputs["score_thr"])).any(), "no score exactly on the threshold"
    if a >= 1023:
        assert valid[0] == min(mt, c * mpc)
        assert AC.inverted(AC.oracle_corners(inputs)).mean() >= 0.25


def test_bound_case_is_quick_and_not_empty():
    inputs, _ = AC.nms_bound()
    assert inputs["probs"].shape == (1, 150000, 2)
    out, valid = AC.oracle_nms(inputs)
    assert valid[0] == 8
    idx_hi = np.flatnonzero(inputs["probs"][0, :, 1] > F32(inputs["score_thr"]))
    assert idx_hi.max() > 140000, "no candidate near the end of the anchor range"


# ---------------------------------------------------------------------------------------------------------------- encode
@pytest.mark.parametrize("thr", [0.5, AC.HALF_BELOW])
def test_hand_built_encode_set(thr):
    inputs, _ = AC.encode_hand(thr)
    iou = AC.iou_plus1(AC.HAND_ANCHORS, AC.HAND_GT)
    assert iou[0, 0] == F32(0.5)                           # exactly on the threshold
    assert not iou[:, 1].any()                             # a ground truth that overlaps nothing
    assert iou[1, 0] == iou[2, 0] == 1                     # duplicate anchors
    assert np.argmax(iou[:, 2]) == np.argmax(iou[:, 3]) == 4 and np.argmax(iou[4]) == 2     # shared best anchor, its own best is the earlier one
    _, _, match = AC.oracle_encode(inputs, 0)
    assert match.tolist() == AC.HAND_MATCH[thr]
    _, _, match_rev = AC.oracle_encode(inputs, 1)          # rows reversed: gt 3 -> row 0, gt 2 -> row 1, gt 0 -> row 3
    assert match_rev.tolist() == [{-1: -1, 0: 3, 3: 1}[m] if d != 4 else 1 for d, m in enumerate(AC.HAND_MATCH[thr])]
    labels, boxes, match_empty = AC.oracle_encode(inputs, 2)
    assert (match_empty == -1).all() and (labels[:, 0] == 1).all() and not boxes.any()


@pytest.mark.parametrize("name", [n for n in AC.ENCODE_CASES if not n.startswith("hand")])
def test_encode_cases_use_both_matching_steps(name):
    inputs, _ = AC.ENCODE_CASES[name]()
    anchors, gmax = inputs["anchors"], inputs["gmax"]
    only1 = only2 = empty = 0
    for i in range(inputs["cnt"].size):
        g = min(int(inputs["cnt"][i]), gmax)
        gt = inputs["gt"][i, :g]
        empty += g == 0
        if g == 0:
            continue
        iou = AC.iou_plus1(anchors, gt)
        assert np.isfinite(iou).all()
        assert (gt[:, 0] >= 1).all() and (gt[:, 0] < inputs["c"]).all()
        s1, s2 = AC.encode_steps(anchors, gt, inputs["thr"])
        _, _, match = AC.oracle_encode(inputs, i)
        assert np.array_equal(match >= 0, s1 | s2)
        only1 += int((s1 & ~s2).sum())
        only2 += int((s2 & ~s1).sum())
    assert only1 >= 1 and only2 >= 1 and empty >= 1, (only1, only2, empty)


def test_encode_case_specifics():
    inputs, _ = AC.encode_gmax64()
    assert inputs["cnt"].tolist() == [64, 63, 1, 0] and inputs["gmax"] == 64
    inputs, _ = AC.encode_1025()
    assert inputs["anchors"].shape[0] == 1025 and AC.oracle_encode(inputs, 2)[2][1024] == 4
    inputs, _ = AC.encode_far_twin()
    assert np.array_equal(inputs["anchors"][7], inputs["anchors"][1030])
    m = AC.oracle_encode(inputs, 0)[2]
    assert m[7] == 1 and m[1030] == 1                      # the twin is matched too, but only through the threshold
    s1, _ = AC.encode_steps(inputs["anchors"], inputs["gt"][0], 0.5)
    assert s1[7] and not s1[1030]
    inputs, _ = AC.encode_overfull()
    assert inputs["cnt"][0] > inputs["gmax"] == inputs["gt"].shape[1]
    inputs, _ = AC.encode_cropped()
    gt = inputs["gt"][0, :inputs["cnt"][0]]
    assert (gt[:, 1] == gt[:, 3]).sum() >= 3 and (gt[:, 2] == gt[:, 4]).sum() >= 2
    assert gt[:, 1:].min() == 0 and gt[:, 3].max() == 639 and gt[:, 4].max() == 479
    for c in (2, 4, 7):
        inputs, _ = AC.encode_ragged(c)
        assert inputs["anchors"].shape[0] == 188
        labels = {int(v) for i in (0, 2) for v in inputs["gt"][i, :inputs["cnt"][i], 0]}
        assert max(labels) == c - 1


# --------------------------------------------------------------------------------------------------- segmentation suppression
@pytest.mark.parametrize("name", AC.SEG_CASES)
def test_seg_cases(name):
    inputs, _ = AC.seg_case(name)
    mask, probs = inputs["mask"], inputs["probs"]
    present = AC.SEG_PRESENT[name]
    out = O.seg_suppress(mask, probs)
    assert (probs > 0).all()
    assert [bool(out[:, k].any()) for k in range(4)] == [bool(p) for p in present]
    npix = mask.shape[1]
    if name.endswith("last-pixel"):
        cls = mask[0].argmax(-1)
        assert (cls[:-1] != cls[-1]).all()                 # that class nowhere else
    if name == "63-ties":
        assert mask[0, 40, 1] == mask[0, 40, 2] == mask[0, 40, 3] and mask[0, 62, 2] == mask[0, 62, 3]
        assert (mask[0].argmax(-1) == 1).sum() == 1 and (mask[0].argmax(-1) == 2).sum() == 1
    assert (npix, probs.shape[0]) in [(1, 1), (63, 255), (65, 255), (257, 1), (AC.GRID + 3, 255), (257, AC.GRID + 1)]


# ---------------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("count", AC.ADAM_COUNTS[:-1])
def test_adam_cases_move_far_more_than_they_round(count):
    inputs, _ = AC.adam_case(count, 50)
    g = inputs["g"]
    nz = np.abs(g[g != 0])
    assert (g == 0).any() and nz.min() < 1e-5 and nz.max() > 1.0 if count > 1 else nz.size > 0
    p64, _, _ = AC.adam_oracle(inputs, 1, 1.0, np.float64)
    p32, m32, v32 = AC.adam_oracle(inputs, 1, 1.0, np.float32)
    assert p32.dtype == np.float32 and m32.dtype == np.float32
    moved = np.abs(p64 - inputs["p"]).max()
    e32 = np.abs(p32.astype(np.float64) - p64).max()
    assert moved > (0.05 if count > 100 else 1e-3) and e32 < 1e-3 * moved
