#!/usr/bin/env python3
"""Wall time of the test-set evaluation of NB03#cell21-29 on one synthetic test set at 480x640, over a 3 x 3 grid of NMS
thresholds and three AP thresholds:
  (a) the host path: per grid pair an inference model and a full `predict` pass over the expanded float32 images (every output
      downloaded, the (N, 480, 640, 4) masks included), `average_precision_object_detection` per AP threshold on the detections
      (ground truth through CSV files, as the function reads it), and once the soft Jaccard of the masks in NumPy (the arithmetic
      of `jaccard_iou_semantic_segmentation` on arrays; PNG decoding is left out, in (a)'s favour);
  (b) one `evaluators.evaluate_on_device` call on the same samples in a ResidentDataset with the same grid.
Path (a) uses nothing this call added, so it is also the figure of the code before it.  The two alternate, `repeats` times, after
one warm-up of each (engines lowered, code objects loaded); every timed region ends in a download, i.e. synchronised.
usage: python scripts/eval_path_time.py [samples=64] [batch=16] [repeats=3]"""
import os, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "multi-task-learning-object-detection-semantic-segmentation_amd"))
import numpy as np
import bench
import ssdseglib
from ssdseglib import _engine as E, _hip as H, evaluators

samples = int(sys.argv[1]) if len(sys.argv) > 1 else 64
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 16
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
GRID = [(b, p) for b in (0.3, 0.45, 0.6) for p in (0.26, 0.3, 0.4)]
AP_THRESHOLDS = (0.5, 0.75, 0.9)
LABELS_CODES, BACKGROUND = [0, 1, 2, 3], 0
NMS = dict(max_number_of_boxes_per_class=10, max_number_of_boxes_per_sample=20, suppress_background_boxes=False, use_segmentation_suppression=True)

ctx = H.Context(0)
E.set_default_context(ctx)
boxes, builder = bench.build_models()
model = builder.get_model_for_training('deeplabv3plus', 'ssdlite', segmentation_dilation_rates=(3, 6, 12))
images = bench.synthetic_images(samples, 1993).astype(np.uint8)
gt, cnt, onehot = bench.synthetic_ground_truth(samples, 11)
index = onehot.argmax(-1).astype(np.uint8)
del onehot
gts = [gt[i, :cnt[i]] for i in range(samples)]
enc = ssdseglib.datacoder.DataEncoderDecoder(
    4, bench.IMAGE_SHAPE[:2], xmin_boxes_default=boxes.get_boxes_coordinates_xmin('ssd'), ymin_boxes_default=boxes.get_boxes_coordinates_ymin('ssd'),
    xmax_boxes_default=boxes.get_boxes_coordinates_xmax('ssd'), ymax_boxes_default=boxes.get_boxes_coordinates_ymax('ssd'),
    iou_threshold=0.525, standard_deviations_centroids_offsets=bench.STDS)
ds = ssdseglib.datacoder.ResidentDataset(enc, zip(images, index, gts), batch_size=batch, shuffle=False)
tmp = tempfile.mkdtemp()
csvs = []
for i, g in enumerate(gts):
    csvs.append(os.path.join(tmp, f"{i}.csv"))
    with open(csvs[-1], "w") as f:
        f.writelines(f"{int(r[0])},{float(r[1])!r},{float(r[2])!r},{float(r[3])!r},{float(r[4])!r}\n" for r in g)
inference = {pair: builder.get_model_for_inference(model_trained=model, boxes_iou_threshold=pair[0], labels_probability_threshold=pair[1], **NMS)
             for pair in GRID}


def host_path(n):
    """NB03#cell21-29 the slow way on the first n samples -> (iou, ap, detections) shaped like evaluate_on_device's result"""
    x = [images[lo:lo + batch].astype(np.float32) for lo in range(0, n, batch)]       # read_and_encode's float images
    ap, dets, masks = {}, {}, None
    for pair in GRID:
        masks, det = inference[pair].predict(x)
        dets[pair] = det
        ap[pair] = {t: evaluators.average_precision_object_detection(list(det[..., 0].astype(np.int32)), list(det[..., 1]), list(det[..., 2:]), t,
                                                                      csvs[:n], LABELS_CODES, BACKGROUND) for t in AP_THRESHOLDS}
    true = (index[:n, ..., None] == np.arange(4)).astype(np.float32)
    inter = (true * masks).sum(axis=(1, 2))
    total = (true + masks).sum(axis=(1, 2))
    iou = (inter / (total - inter + np.float32(1e-7))).mean(axis=0)
    return {l: float(v) for l, v in zip(LABELS_CODES, iou) if l != BACKGROUND}, ap, dets


def device_path(n):
    data = ds if n == samples else [ds.batch(np.arange(lo, min(lo + batch, n))) for lo in range(0, n, batch)]
    r = evaluators.evaluate_on_device(inference[GRID[0]], data, LABELS_CODES, BACKGROUND, AP_THRESHOLDS, nms_grid=GRID)
    return r["iou"], r["ap"], r["detections"]


# warm-up on one batch of every size the timed passes use, and the agreement of the two paths on it
for n in sorted({batch, samples % batch or batch}):
    a, b = host_path(n), device_path(n)
    same = all(np.array_equal(a[2][p], b[2][p]) for p in GRID)
    print(f"warm-up on {n} samples: detections {'bit-identical' if same else 'DIFFER'}, AP {'equal' if a[1] == b[1] else 'DIFFER'}, "
          f"max |iou difference| {max(abs(a[0][l] - b[0][l]) for l in a[0]):.2e}, "
          f"{sum(int((a[2][p][..., 0] > 0).sum()) for p in GRID)} non-background detections over the grid")
times = {"host": [], "device": []}
for _ in range(repeats):
    for name, fn in (("host", host_path), ("device", device_path)):
        ctx.sync()
        t0 = time.perf_counter()
        fn(samples)
        times[name].append(time.perf_counter() - t0)
for name, t in times.items():
    print(f"{name:6s} path, {samples} samples of 480x640 in batches of {batch}, {len(GRID)} NMS pairs x {len(AP_THRESHOLDS)} AP thresholds: "
          f"median {np.median(t):.3f} s ({1e3 * np.median(t) / samples:.1f} ms/sample), repeats {' '.join(f'{v:.3f}' for v in t)}")
print(f"host / device (medians): {np.median(times['host']) / np.median(times['device']):.1f}x  (device: {ctx.device_name()})")
