"""Test-set evaluation on the device (csrc/evaluate.hip, evaluators.evaluate_on_device; reference NB03#cell21-29).

1. ssdseg_eval_mask_jaccard against a float64 restatement of evaluators.jaccard_iou_semantic_segmentation's arithmetic (2e-4
   absolute, the bound tests/test_gpu_eval_surface.py uses for metrics of this form against float64), twice with equal bits, in
   guarded buffers: the dword / float4 path with heads and tails (hw = 35: images 1 and 2 start 3 and 2 bytes off a dword), several
   blocks per image, c = 3 (the plain path), and the same c = 4 case with the class indices one byte off a dword and with the
   probabilities 4 bytes off 16 (the plain path for c = 4).
2. ssdseg_eval_det_best_iou against evaluators._iou_boxes_pred_vs_true(...).max(axis=1) (1e-6: both sides evaluate the same
   float32 expressions), ground-truth counts 0, 1, 3 and GMAX with decoy rows past the count.
3. evaluate_on_device end to end on the small model after a few training steps, 3 samples cut 2 + 1, from CompactBatch objects and
   from a ResidentDataset, with and without segmentation suppression: detections bit-identical to predict on the same batches of
   float images, the Jaccard within 2e-4 of the float64 restatement on predict's mask output, AP equal (1e-12) to
   average_precision_object_detection fed predict's detections and the ground truth through CSV files.
4. A grid of two NMS threshold pairs: each pair's detections are those of a fresh inference model built with that pair; the
   network ran once per batch.
5. Nothing larger than one batch's detection rows is downloaded.
"""
import numpy as np
import pytest

from tests.test_gpu_eval_surface import compile_model, perturbed_moving_statistics
from tests.test_gpu_full_model import SHAPE, build, make_targets
from tests.test_gpu_training_steps import randomise_bn
from _guard import guards  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

JACCARD_TOL = 2e-4
BEST_IOU_TOL = 1e-6
LABELS_CODES, BACKGROUND = [0, 1, 2, 3], 0


def jaccard_f64(prob, index):
    """evaluators.py:84-96 before the mean over the samples, in float64: (n, c)"""
    n, c = prob.shape[0], prob.shape[-1]
    pred = np.asarray(prob, np.float64).reshape(n, -1, c)
    true = (np.asarray(index, np.int64).reshape(n, -1, 1) == np.arange(c)).astype(np.float64)
    inter = (true * pred).sum(axis=1)
    total = (true + pred).sum(axis=1)
    return inter / (total - inter + 1e-7)


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------ 1. the Jaccard kernel
@pytest.mark.parametrize("shape,mask_off,prob_off", [((3, 5, 7, 4), 0, 0), ((2, 64, 96, 4), 0, 0), ((2, 9, 11, 3), 0, 0),
                                                     ((3, 5, 7, 4), 1, 0), ((3, 5, 7, 4), 0, 1)])
def test_mask_jaccard_kernel(ctx, guards, shape, mask_off, prob_off):
    n, h, w, c = shape
    hw = h * w
    rng = np.random.default_rng(7)
    prob = softmax(rng.normal(0, 1.5, (n, hw, c))).astype(np.float32)
    index = rng.integers(0, c + 2, (n, hw)).astype(np.uint8)          # c and c + 1: all-zero one-hot pixels
    index[0, ::5] = 255
    index[-1][index[-1] == 1] = 0                                      # the last image lacks class 1: I = 0 there
    want = jaccard_f64(prob, index)
    assert want[-1, 1] == 0 and (index >= c).any() and (want[:-1] > 0).all()

    d_prob = guards.inp(np.concatenate([np.zeros(prob_off, np.float32), prob.ravel()]))
    d_index = guards.inp(np.concatenate([np.zeros(mask_off, np.uint8), index.ravel()]))
    p_view, i_view = d_prob.view(prob_off, (n, hw, c)), d_index.view(mask_off, (n, hw))
    outs = [guards.out((n, c)), guards.out((n, c))]
    for out in outs:
        ctx.call("ssdseg_eval_mask_jaccard", p_view, i_view, n, hw, c, out)
    got = [out.download() for out in outs]
    assert guards.unwritten(outs[0]).size == 0 and guards.unwritten(outs[1]).size == 0
    err = np.abs(got[0].astype(np.float64) - want).max()
    print(f"jaccard {shape} mask+{mask_off} prob+{prob_off}: max |device - float64| = {err:.3e}")
    assert err < JACCARD_TOL, (got[0], want)
    assert got[0][-1, 1] == 0
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "two runs, two results"


def test_mask_jaccard_kernel_rejects_bad_arguments(ctx, guards):
    from ssdseglib._hip import SsdsegError
    prob, index, out = guards.inp(np.zeros((1, 4, 4), np.float32)), guards.inp(np.zeros((1, 4), np.uint8)), guards.out((1, 4))
    for args, code in (((prob, index, 1, 4, 0, out), -1006), ((prob, index, 1, 4, 9, out), -1006), ((prob, index, 0, 4, 4, out), -1004),
                       ((prob, index, 1, 0, 4, out), -1005), ((prob, None, 1, 4, 4, out), -1003)):
        with pytest.raises(SsdsegError, match=str(code)):
            ctx.call("ssdseg_eval_mask_jaccard", *args)
    ctx.call("ssdseg_eval_mask_jaccard", prob, index, 1, 4, 4, out)      # (the output is written in the end: no poison at teardown)
    assert guards.unwritten(out).size == 0


# ------------------------------------------------------------------------------------------------------ 2. the best-IoU kernel
def test_det_best_iou_kernel(ctx, guards):
    from ssdseglib import evaluators
    from ssdseglib._loaders import _CompactLoader
    n, r, gmax = 4, 10, _CompactLoader.GMAX
    rng = np.random.default_rng(11)
    counts = np.array([0, 1, 3, gmax], np.int32)
    gt = np.zeros((n, gmax, 5), np.float32)
    x0, y0 = rng.uniform(0, 500, (n, gmax)), rng.uniform(0, 380, (n, gmax))
    gt[..., 0] = rng.integers(1, 4, (n, gmax))
    gt[..., 1], gt[..., 2] = x0, y0
    gt[..., 3], gt[..., 4] = x0 + rng.uniform(8, 120, (n, gmax)), y0 + rng.uniform(8, 90, (n, gmax))
    for i, k in enumerate(counts):                       # decoys past the count: every label, the whole image
        gt[i, k:] = [1, 0, 0, 640, 480]
        gt[i, k + 1::3, 0] = 2
        gt[i, k + 2::3, 0] = 3
    det = np.zeros((n, r, 6), np.float32)
    for i in range(n):
        g = gt[i, 0] if counts[i] else np.array([1, 100, 100, 200, 180], np.float32)
        other = 1 + (int(g[0]) % 3)
        det[i, 0] = [g[0], 0.9, *g[1:]]                                  # an exact match (where the image has ground truth)
        det[i, 1] = [other, 0.8, *g[1:]]                                 # the same box under another label
        det[i, 2] = [0, 0.7, *g[1:]]                                     # label 0 on top of a ground-truth box
        det[i, 3] = [g[0], 0.6, 2000, 2000, 2040, 2030]                  # disjoint from everything
        for j in range(4, r - 1):                                        # shifted copies of ground-truth boxes, any label
            s = gt[i, rng.integers(0, max(int(counts[i]), 1))]
            det[i, j] = [rng.integers(0, 4), rng.uniform(0.1, 0.5), *(s[1:] + rng.normal(0, 12, 4))]
        # the last row stays zero: an empty NMS row
    want = np.zeros((n, r), np.float32)
    for i, k in enumerate(counts):
        want[i] = evaluators._iou_boxes_pred_vs_true(det[i, :, 0], det[i, :, 2:], gt[i, :k, 0], gt[i, :k, 1:]).max(axis=1)
    want[det[..., 0] == 0] = 0                            # (the host evaluator drops these rows before it computes an IoU)
    assert (want[1:, 0] > 0.999).all() and want[1, 1] == 0 and (want[:, 3] == 0).all() and not want[0].any()
    assert ((want > 0.05) & (want < 0.95)).sum() >= 5, "partial overlaps too"

    out = guards.out((n, r))
    ctx.call("ssdseg_eval_det_best_iou", guards.inp(det), guards.inp(gt), guards.inp(counts), n, r, gmax, out)
    got = out.download()
    assert guards.unwritten(out).size == 0
    err = np.abs(got - want).max()
    print(f"best IoU: max |device - host| = {err:.3e}; exact matches {got[1:, 0]}")
    assert err <= BEST_IOU_TOL, (got, want)
    assert not got[0].any() and not got[det[..., 0] == 0].any(), "no ground truth / label 0: exactly 0"


# ------------------------------------------------------------------------------------------------------ 3 - 5. end to end
P_THRESHOLD = 0.05       # labels_probability_threshold of the model under test: low enough for non-background detections (asserted)
B_THRESHOLD = 0.3
NMS = dict(max_number_of_boxes_per_class=8, max_number_of_boxes_per_sample=20, suppress_background_boxes=False)
R = NMS["max_number_of_boxes_per_sample"]


@pytest.fixture(scope="module")
def trained(ctx):
    """the small model of tests/test_gpu_full_model.py after three training steps, and three test samples as the files hold them"""
    import ssdseglib
    from ssdseglib import _engine as E
    E.set_default_context(ctx)
    rng = np.random.default_rng(1993)
    boxes, builder, model = build(seed=5)
    randomise_bn(model, rng)
    x = rng.integers(0, 256, (3,) + SHAPE).astype(np.float32)
    perturbed_moving_statistics(model, rng, x)
    compile_model(model, boxes, lr=1e-3)
    _, _, targets = make_targets(rng, boxes, 3)
    for _ in range(3):
        logs = model.train_on_batch(x, targets)
    assert np.isfinite(logs["loss"])
    enc, _, t = make_targets(rng, boxes, 3)
    images = rng.integers(0, 256, (3,) + SHAPE).astype(np.uint8)
    index = t['output-mask'].argmax(-1).astype(np.uint8)
    index[:, :2, :5] = 7                                                # a class index the model does not have
    out = dict(builder=builder, model=model, enc=enc, images=images, index=index, datacoder=ssdseglib.datacoder)
    out["gts"] = ground_truth_near_the_detections(out, rng)
    return out


def ground_truth_near_the_detections(trained, rng):
    """Ground truth the model partly hits, so that AP is not 0 across the board: per image up to three of its non-background
    detections with a proper extent become ground-truth boxes of the same label -- the first moved by a pixel or two (IoU near
    0.9), the second by a quarter of its width (near 0.6), the third by half of it (near 0.33) -- plus one box of another label
    on top of the first detection; an image without such a detection gets one box away from everything."""
    _, det = predict_batches(inference_model(trained, True), trained)
    gts, used = [], 0
    for i, d in enumerate(det):
        rows = [r for r in d if r[0] > 0 and r[4] - r[2] > 8 and r[5] - r[3] > 8][:3]
        g = []
        for k, r in enumerate(rows):
            w = r[4] - r[2]
            dx = (rng.uniform(-2, 2), w / 4, w / 2)[k]
            g.append([r[0], r[2] + dx, r[3] + rng.uniform(-2, 2), r[4] + dx, r[5] + rng.uniform(-2, 2)])
        if rows:
            g.append([1 + int(rows[0][0]) % 3, *rows[0][2:]])
        if not g:
            g.append([1 + i % 3, 5, 5, 40, 30])
        used += len(rows)
        gts.append(np.asarray(g, np.float32))
    print("proper non-background detections used:", used, "ground-truth rows per image:", [len(g) for g in gts], "confidences of the non-background rows:",
          np.sort(det[..., 1][det[..., 0] > 0]))
    return gts


def inference_model(trained, suppression, b_thr=B_THRESHOLD, p_thr=P_THRESHOLD):
    return trained["builder"].get_model_for_inference(model_trained=trained["model"], boxes_iou_threshold=b_thr, labels_probability_threshold=p_thr,
                                                      use_segmentation_suppression=suppression, **NMS)


def compact_batches(trained):
    d, cut = trained, ((0, 2), (2, 3))
    return [d["datacoder"].CompactBatch(d["images"][a:b], d["index"][a:b], d["gts"][a:b], None, d["enc"]) for a, b in cut]


def resident_dataset(trained):
    d = trained
    return d["datacoder"].ResidentDataset(d["enc"], zip(d["images"], d["index"], d["gts"]), batch_size=2, shuffle=True, seed=3)


def predict_batches(model, trained):
    x = trained["images"].astype(np.float32)
    return model.predict([x[:2], x[2:]])


def ap_thresholds(best):
    """three AP thresholds at least 1e-3 away from every best-IoU value that occurs"""
    out = []
    for t in (0.25, 0.5, 0.75):
        while best.size and np.abs(best - t).min() < 2e-3:
            t += 1e-3
        out.append(t)
    return out


def write_csvs(tmp_path, gts):
    paths = []
    for i, g in enumerate(gts):
        p = tmp_path / f"gt{i}.csv"
        p.write_text("".join(f"{int(r[0])},{float(r[1])!r},{float(r[2])!r},{float(r[3])!r},{float(r[4])!r}\n" for r in g))
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("suppression", [True, False])
@pytest.mark.parametrize("source", ["compact", "resident"])
def test_evaluate_on_device_end_to_end(ctx, guards, tmp_path, trained, suppression, source):
    from ssdseglib import _engine as E, evaluators
    E.set_default_context(ctx)
    model = inference_model(trained, suppression)
    seg, det = predict_batches(model, trained)
    assert seg.shape == (3,) + SHAPE[:2] + (4,) and det.shape == (3, R, 6)
    n_fg = int((det[..., 0] > 0).sum())
    print(f"suppression={suppression}: {n_fg} non-background detections, {int((det[..., 1] > 0).sum())} in all")
    assert n_fg > 0, "no non-background detection: lower P_THRESHOLD"

    gts = trained["gts"]
    best = np.concatenate([evaluators._iou_boxes_pred_vs_true(d[:, 0], d[:, 2:], g[:, 0], g[:, 1:]).max(axis=1)[d[:, 0] > 0] for d, g in zip(det, gts)])
    thresholds = ap_thresholds(best)
    assert all(np.abs(best - t).min() >= 1e-3 for t in thresholds), (thresholds, best)

    data = compact_batches(trained) if source == "compact" else resident_dataset(trained)
    result = evaluators.evaluate_on_device(model, data, LABELS_CODES, BACKGROUND, thresholds)
    pair = (B_THRESHOLD, P_THRESHOLD)
    assert set(result) == {"iou", "ap", "detections"} and set(result["detections"]) == {pair} and set(result["ap"]) == {pair}
    got_det = result["detections"][pair]
    assert got_det.shape == det.shape and got_det.dtype == np.float32
    assert np.array_equal(got_det.view(np.uint32), det.view(np.uint32)), "detections differ from predict on the same batches"

    want_iou = jaccard_f64(seg, trained["index"]).mean(axis=0)
    assert set(result["iou"]) == {1, 2, 3}
    for l in (1, 2, 3):
        print(f"  iou[{l}]: device {result['iou'][l]!r} float64 on predict's masks {want_iou[l]!r}")
        assert abs(result["iou"][l] - want_iou[l]) < JACCARD_TOL

    paths = write_csvs(tmp_path, gts)
    assert set(result["ap"][pair]) == set(thresholds)
    for t in thresholds:
        want = evaluators.average_precision_object_detection(list(det[..., 0].astype(np.int32)), list(det[..., 1]), list(det[..., 2:]), t, paths,
                                                             LABELS_CODES, BACKGROUND)
        got = result["ap"][pair][t]
        print(f"  ap at {t}: device {got} host {want}")
        assert set(got) == set(want) == {1, 2, 3}
        assert all(abs(got[l] - want[l]) <= 1e-12 for l in want), (t, got, want)
    values = {t: tuple(result["ap"][pair][t][l] for l in (1, 2, 3)) for t in thresholds}
    print(f"  AP per threshold (classes 1, 2, 3): {values}")


def test_resident_dataset_is_walked_in_slot_order_and_left_alone(ctx, guards, trained):
    """shuffle=True and an encoder that flips: evaluation still takes the samples as stored, and the dataset's generator is where
    it was (the next epoch it plans is the one a twin with the same seed plans first)"""
    from ssdseglib import _engine as E, evaluators
    E.set_default_context(ctx)
    model = inference_model(trained, True)
    ds, twin = resident_dataset(trained), resident_dataset(trained)
    a = evaluators.evaluate_on_device(model, ds, LABELS_CODES, BACKGROUND, [0.5])
    b = evaluators.evaluate_on_device(model, [ds.batch([0, 1]), ds.batch([2])], LABELS_CODES, BACKGROUND, [0.5])
    c = evaluators.evaluate_on_device(model, [ds.batch([1, 0]), ds.batch([2])], LABELS_CODES, BACKGROUND, [0.5])      # gathered class indices
    pair = (B_THRESHOLD, P_THRESHOLD)
    assert np.array_equal(a["detections"][pair], b["detections"][pair]) and a["iou"] == b["iou"] and a["ap"] == b["ap"]
    assert np.array_equal(c["detections"][pair][[1, 0, 2]], a["detections"][pair]) and a["ap"] == c["ap"]
    assert all(abs(a["iou"][l] - c["iou"][l]) < 1e-6 for l in a["iou"])
    assert [tuple(x.index) for x in ds] == [tuple(x.index) for x in twin]


def test_threshold_grid_runs_the_network_once_per_batch(ctx, guards, trained, monkeypatch):
    from ssdseglib import _engine as E, evaluators
    E.set_default_context(ctx)
    grid = [(0.3, P_THRESHOLD), (0.6, 0.6)]
    want = {pair: predict_batches(inference_model(trained, True, *pair), trained)[1] for pair in grid}
    print("detection rows that differ between the two pairs:", int((want[grid[0]] != want[grid[1]]).any(-1).sum()))
    model = inference_model(trained, True, 0.45, 0.5)                   # its own pair is not in the grid
    calls = {"forward": 0, "decode": 0, "nms": 0}

    def counted(cls, name, key):
        real = getattr(cls, name)

        def wrapper(self, *a, **k):
            calls[key] += 1
            return real(self, *a, **k)
        monkeypatch.setattr(cls, name, wrapper)

    counted(E.Engine, "forward", "forward")
    counted(E.DecodeNmsOp, "decode", "decode")
    counted(E.DecodeNmsOp, "run_nms", "nms")
    result = evaluators.evaluate_on_device(model, compact_batches(trained), LABELS_CODES, BACKGROUND, [0.5], nms_grid=grid)
    assert calls == {"forward": 2, "decode": 2, "nms": 4}, calls
    assert list(result["detections"]) == grid
    for pair in grid:
        assert np.array_equal(result["detections"][pair].view(np.uint32), want[pair].view(np.uint32)), pair


def test_no_large_download(ctx, guards, trained, monkeypatch):
    from ssdseglib import _engine as E, _hip as H, evaluators
    E.set_default_context(ctx)
    model = inference_model(trained, True)
    sizes = []
    real = H.DeviceBuffer.download

    def download(self):
        sizes.append(self.nbytes)
        return real(self)

    monkeypatch.setattr(H.DeviceBuffer, "download", download)
    evaluators.evaluate_on_device(model, compact_batches(trained), LABELS_CODES, BACKGROUND, [0.5], nms_grid=[(0.3, 0.3), (0.5, 0.1)])
    n, r = 2, R
    mask_bytes = n * SHAPE[0] * SHAPE[1] * 4 * 4
    print(f"downloads: {len(sizes)}, largest {max(sizes)} bytes (one batch's mask output: {mask_bytes})")
    assert sizes and max(sizes) <= n * r * 6 * 4 < mask_bytes
