"""The input side of an `_engine.Engine`: a loader fills the engine's input and target buffers from one batch, in two phases.

  * `stage(x, y)` is the host side.  It may run while the previous step is still on the GPU (`ahead=True`: fit's look-ahead).
  * `consume()` is the device side, at the start of the step that uses the batch.
  * `stages_ahead` says whether staging ahead buys anything: uploads on the context's copy stream do, a resident batch does not.

One loader class per kind of batch, picked and cached by `loader_for`: dense `(x, y)` arrays, `datacoder.CompactBatch`,
`datacoder.ResidentBatch`.  Their upload_sync / upload_async(after_fence=True) / upload_join / upload_fence order is the copy-stream protocol.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _hip as H
from ._batches import GMAX, pad_ground_truth


def batch_size(x) -> int:
    return len(x) if hasattr(x, "__len__") else int(x.shape[0])


def _pad_ground_truth(ground_truth, b, gmax):
    """the b per-image (k_i, 5) rows of a compact batch -> gt (b, gmax, 5) float32, zero-padded, and cnt (b,) int32"""
    if max(g.shape[0] for g in ground_truth) > gmax:
        raise ValueError(f"more than {gmax} ground-truth boxes in one image")
    return pad_ground_truth(ground_truth, gmax)


class _DenseLoader:
    """Dense `(x, y)` arrays.  Staged at the start of their own step they go straight into the engine's buffers (`set_input` /
    `set_targets`, synchronous).  Staged AHEAD, the host arrays are uploaded on the context's copy stream into device staging
    buffers while the GPU computes the current step (the host thread blocks in the copy -- the runtime pipelines pageable memory
    through its own pinned buffers at ~45 GB/s -- but it has nothing else to do until the step's losses are ready); consume() makes
    the main stream wait for that upload and copies staging -> the engine's buffers (device to device, ~0.3 ms for 285 MB).  The
    engine's own buffers cannot be the upload target: the running step still reads them (the mask targets until the end of the
    backward pass).  Pinned host buffers of the loader's own bought nothing: that host memcpy took as long as the step."""

    stages_ahead = True

    def __init__(self, eng, encoder=None):
        self.eng, self.ctx, self.enc = eng, eng.ctx, None
        self.names = [r.name for r in eng._loss_names]
        self.dst = [eng.input_store.buf] + [r.target for r in eng._loss_names]
        self.staging = None     # device staging buffers, allocated by the first look-ahead
        self.staged = None      # True: an upload is in flight; an (x, y) pair: consume() takes the synchronous path
        self._keep = None       # the host arrays of the upload in flight

    def stage(self, x, y=None, ahead=False) -> bool:
        """False: this batch cannot go ahead (device buffers, another size); it is staged again at the start of its own step"""
        if not ahead:
            self.staged = (x, y)
            return True
        arrays = [x] + [y[name] for name in self.names]
        if any(isinstance(a, H.DeviceBuffer) for a in arrays) or any(int(np.prod(np.shape(a))) != d.size for a, d in zip(arrays, self.dst)):
            return False
        if self.staging is None:
            self.staging = [self.ctx.empty(d.shape) for d in self.dst]
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]   # no copy for float32 C-contiguous batches
        self.ctx.upload_sync()
        for a, st in zip(arrays, self.staging):
            self.ctx.upload_async(st, a, after_fence=True)   # behind the last consume(), under the step queued after it
        self._keep = arrays
        self.staged = True
        return True

    def consume(self) -> None:
        assert self.staged is not None
        if self.staged is True:                         # staging -> the engine's buffers
            self.ctx.upload_join()
            for d, st in zip(self.dst, self.staging):
                d.copy_from(st)
            self.ctx.upload_fence()                     # from here on the staging buffers may be overwritten
        else:
            x, y = self.staged
            self.eng.set_input(x)
            if y is not None:
                self.eng.set_targets(y)
        self.staged = None


def _encoder_anchors(ctx, encoder, det, mask_op):
    """the encoder's default boxes on the device, after checking its anchor and class counts against the model's heads"""
    anchors = ctx.array(encoder._corners())
    if det is not None and anchors.shape[0] != det.y_boxes.shape[1]:
        raise ValueError(f"encoder has {anchors.shape[0]} default boxes, the model's heads {det.y_boxes.shape[1]}")
    # ssdseg_encode_targets writes (batch, anchors, encoder.num_classes) floats into the labels target and the mask is
    # expanded to encoder.num_classes planes (reference datacoder.py:332): both buffers are sized by the MODEL's channels
    if det is not None and int(encoder.num_classes) != det.y_labels.shape[-1]:
        raise ValueError(f"encoder.num_classes = {encoder.num_classes}, the model's labels head has {det.y_labels.shape[-1]} classes")
    if mask_op is not None and int(encoder.num_classes) != mask_op.y_true.shape[-1]:
        raise ValueError(f"encoder.num_classes = {encoder.num_classes}, the model's mask head has {mask_op.y_true.shape[-1]} classes")
    return anchors


class _CropStage:
    """The geometric step of both loaders: a batch that carries crop windows (csrc/crop.hip) or a mosaic (csrc/mosaic.hip) is cropped
    or assembled, uint8 -> uint8, into ONE set of device staging buffers -- pixels, class indices, ground-truth rows, counts: an
    ordinary compact batch -- and the compact-path calls then run on those.  Crop or mosaic first, then flip, then colour.  The
    buffers are allocated on first use."""

    def __init__(self, ctx, b, h, w, gmax):
        self.ctx, self.b, self.h, self.w, self.gmax = ctx, b, h, w, gmax
        self.img = ctx.empty((b, h, w, 3), np.uint8)
        self.midx = ctx.empty((b, h, w), np.uint8)
        self.flip = ctx.empty(b, np.uint8)
        self.gt = ctx.empty((b, gmax, 5))
        self.cnt = ctx.empty(b, np.int32)

    def run(self, src_img, src_midx, src_gt, src_cnt, n_src, index, step, flip_host):
        """step: the batch's `geometric()`, ("crop", windows, fill) or ("mosaic", mosaic, fill); index: the host int32 list of a
        resident batch (its pool slots) or None (n -> n); flip_host: host uint8 flags to hand on to self.flip, or None.  src_midx /
        src_gt may be None (a model without that head)."""
        kind, what, fill = step
        fill = fill if fill is not None else (0, 0, 0, 0)
        if kind == "mosaic":        # the source sample of every tile: the positions within the batch, or the pool slots at those positions
            sources = np.ascontiguousarray(what.index4 if index is None else index[what.index4], np.int32)
            lists = (sources.ctypes.data, what.split.ctypes.data, what.windows.ctypes.data_as(C.POINTER(C.c_float)))
        else:
            lists = (None if index is None else index.ctypes.data, what.ctypes.data_as(C.POINTER(C.c_float)))
        self.ctx.call(f"ssdseg_{kind}_inputs", src_img, src_midx, n_src, *lists, (C.c_uint8 * 3)(*fill[:3]), int(fill[3]),
                      None if flip_host is None else flip_host.ctypes.data, self.flip, self.img, self.midx if src_midx is not None else None,
                      self.b, self.h, self.w)
        if src_gt is not None:
            self.ctx.call(f"ssdseg_{kind}_gt", src_gt, src_cnt, n_src, *lists, self.gt, self.cnt, self.b, self.gmax, self.h, self.w)


class _EncodingLoader:
    """What the compact and the resident loader share: the heads they fill (`mask_op`, `det`: None where the model has no such
    loss), the encoder's anchors, the gt / cnt / means buffers, the crop stage and the compact-path calls.  Without an encoder
    (an inference engine: evaluate) there are no targets: only the image is filled and the ground-truth rows are put into gt / cnt."""

    GMAX = GMAX     # ground-truth rows per image the encode kernel holds in LDS (boxes.hip): the resident dataset's pools have as many

    def __init__(self, eng, encoder):
        self.eng, self.ctx, self.enc = eng, eng.ctx, encoder
        ops = {r.kind: r.op for r in eng._loss_names}
        self.mask_op, self.det = ops.get("mask"), ops.get("conf") or ops.get("loc")
        self.gt = self.ctx.empty((eng.batch, self.GMAX, 5))
        self.cnt = self.ctx.empty(eng.batch, np.int32)
        self.means = self.ctx.empty((eng.batch, 3))      # per-(image, channel) means of the colour augmentation's contrast step
        self.anchors = _encoder_anchors(self.ctx, encoder, self.det, self.mask_op) if encoder is not None else None
        self.staged = None
        self.crop = None

    def _geometric(self, img, midx, gt, cnt, n_src, index, step, flip_host):
        """the batch's geometric step (`geometric()`: crop, mosaic or None), uint8 -> uint8 into a second compact batch on the device
        (the crop stage, allocated on first use), from these source buffers or pools of n_src samples; index, flip_host: as
        _CropStage.run.  -> the compact device buffers (img, midx, gt, cnt) to expand: the stage's, or the sources without a step"""
        if step is None:
            return img, midx, gt, cnt
        if self.crop is None:
            ins = self.eng.input_store
            self.crop = _CropStage(self.ctx, self.eng.batch, ins.h, ins.w, self.GMAX)
        crop = self.crop
        crop.run(img, midx if self.mask_op is not None else None, gt if self.det is not None else None, cnt, n_src, index, step, flip_host)
        return crop.img, crop.midx, crop.gt, crop.cnt

    def _encode(self, gt, cnt) -> None:
        self.ctx.call("ssdseg_encode_targets", self.anchors, self.anchors.shape[0], gt, cnt, self.eng.batch, self.GMAX, self.enc.num_classes,
                      float(self.enc.iou_threshold), (C.c_float * 4)(*self.enc._stds), self.det.y_labels, self.det.y_boxes, None)

    def _expand_compact(self, img, midx, gt, cnt, flip, draws) -> None:
        """the compact path on device buffers: float32 image (cast or colour augmentation), one-hot mask, both mirrored where flagged,
        mirrored boxes, encoded anchors, into the buffers the step reads"""
        ctx, b, ins, mask_op = self.ctx, self.eng.batch, self.eng.input_store, self.mask_op
        c = mask_op.y_true.shape[-1] if mask_op is not None else 1
        if draws is None:
            ctx.call("ssdseg_expand_inputs", img, midx if mask_op is not None else None, flip, ins.buf,
                     mask_op.y_true if mask_op is not None else None, b, ins.h, ins.w, c)
        else:
            ctx.call("ssdseg_rgb_augment", img, flip, (C.c_float * 4)(*draws), self.means, ins.buf, b, ins.h, ins.w)
            if mask_op is not None:
                ctx.call("ssdseg_expand_inputs", None, midx, flip, None, mask_op.y_true, b, ins.h, ins.w, c)
        if self.det is not None:
            if flip is not None:
                ctx.call("ssdseg_flip_gt_boxes", gt, cnt, flip, b, self.GMAX, float(ins.w))
            self._encode(gt, cnt)


class _CompactLoader(_EncodingLoader):
    """A `datacoder.CompactBatch` (reference datacoder.py:302-347 == csrc/inputs.hip + ssdseg_encode_targets).  stage(): 39 MB of
    uint8 pixels / class indices / ground-truth rows go up on the copy stream (under the running step when fit overlaps);
    consume(): the main stream waits for them and expands them (_expand_compact) straight into the buffers the step reads.  Colour
    draws (datacoder.augmentation_rgb_channels) make ssdseg_rgb_augment produce the image instead of the plain cast (reference
    datacoder.py:434-466).  Crop windows (datacoder.augmentation_random_crop) or a mosaic (datacoder.augmentation_mosaic): cropped
    or assembled first, on the device (_CropStage)."""

    stages_ahead = True

    def __init__(self, eng, encoder):
        super().__init__(eng, encoder)
        ctx, b, ins = eng.ctx, eng.batch, eng.input_store
        self.img = ctx.empty((b, ins.h, ins.w, 3), np.uint8)
        self.midx = ctx.empty((b, ins.h, ins.w), np.uint8)
        self.flip = ctx.empty(b, np.uint8)
        self.batch = self._keep = None      # the staged batch (its draws and geometric step are read in consume) and its host arrays

    def stage(self, cb, y=None, ahead=False) -> bool:
        b, ins = self.eng.batch, self.eng.input_store
        if len(cb) != b or cb.images.shape[1:3] != (ins.h, ins.w):
            raise ValueError(f"compact batch {cb.images.shape} for an engine of batch {b}, {ins.h}x{ins.w}")
        gt, cnt = _pad_ground_truth(cb.ground_truth, b, self.GMAX)
        flip = cb.flip if cb.flip is not None else np.zeros(b, np.uint8)
        self.ctx.upload_sync()
        pairs = [(self.img, cb.images), (self.midx, cb.mask_index), (self.gt, gt), (self.cnt, cnt), (self.flip, flip)]
        for dst, src in pairs:
            self.ctx.upload_async(dst, src, after_fence=True)
        self._keep = [src for _, src in pairs]
        self.batch, self.staged = cb, bool(flip.any())
        return True

    def consume(self) -> None:
        assert self.staged is not None
        ctx, cb = self.ctx, self.batch
        ctx.upload_join()
        flip = self.flip if self.staged else None
        compact = self._geometric(self.img, self.midx, self.gt, self.cnt, self.eng.batch, None, cb.geometric(), None)
        self._expand_compact(*compact, flip, cb.rgb_draws)
        ctx.upload_fence()                          # from here on the compact staging buffers may be overwritten
        self.staged = self.batch = None


class _ResidentLoader(_EncodingLoader):
    """A `datacoder.ResidentBatch`: the samples are already in HBM (the dataset's pools), the batch is a list of indices, flip flags
    and colour draws.  stage() keeps the list; consume() builds the batch on the main stream -- ssdseg_gather_inputs (expansion or
    colour augmentation, mirrored where flagged), ssdseg_gather_gt (rows, counts, mirrored boxes), ssdseg_encode_targets -- with
    the bits _CompactLoader gives for `dataset.to_compact(batch)`.  Nothing is uploaded and nothing waits.  Crop windows
    (ResidentDataset(random_crop=...)): cropped from the pools into compact buffers instead (_CropStage takes the index list and
    hands the flip flags on in its kernel arguments), and the compact-path calls run on those.  A mosaic (ResidentDataset(mosaic=...))
    likewise: its positions within the batch become pool slots through the batch's index list."""

    stages_ahead = False

    def stage(self, rb, y=None, ahead=False) -> bool:
        b, ins, ds = self.eng.batch, self.eng.input_store, rb.dataset
        if len(rb) != b or (ds.height, ds.width) != (ins.h, ins.w):
            raise ValueError(f"resident batch of {len(rb)} samples of {ds.height}x{ds.width} for an engine of batch {b}, {ins.h}x{ins.w}")
        if ds.ctx is not self.ctx:
            raise ValueError("resident dataset lives on another context than the model's engine")
        self.staged = rb
        return True

    def consume(self) -> None:
        assert self.staged is not None
        rb, ctx, b, ins, mask_op = self.staged, self.ctx, self.eng.batch, self.eng.input_store, self.mask_op
        ds = rb.dataset
        self.staged = None
        step = rb.geometric()
        if step is not None:
            flip_host = rb.flip if rb.flip is not None and rb.flip.any() else None
            compact = self._geometric(ds.images, ds.masks, ds.gt, ds.cnt, ds.num_samples, rb.index, step, flip_host)
            self._expand_compact(*compact, self.crop.flip if flip_host is not None else None, rb.rgb_draws)
            return
        index = rb.index.ctypes.data
        flip = rb.flip.ctypes.data if rb.flip is not None and rb.flip.any() else None
        draws = (C.c_float * 4)(*rb.rgb_draws) if rb.rgb_draws is not None else None
        c = mask_op.y_true.shape[-1] if mask_op is not None else 1
        ctx.call("ssdseg_gather_inputs", ds.images, ds.masks if mask_op is not None else None, ds.num_samples, index, flip, draws,
                 self.means if draws is not None else None, ins.buf, mask_op.y_true if mask_op is not None else None, b, ins.h, ins.w, c)
        if self.det is not None or self.enc is None:
            ctx.call("ssdseg_gather_gt", ds.gt, ds.cnt, ds.num_samples, index, flip, self.gt, self.cnt, b, self.GMAX, float(ins.w))
        if self.det is not None:
            self._encode(self.gt, self.cnt)


def _pick(eng, x):     # -> (loader class, encoder) for this kind of batch; an engine without compiled losses has nothing to encode
    cls = {"CompactBatch": _CompactLoader, "ResidentBatch": _ResidentLoader}.get(type(x).__name__, _DenseLoader)
    return cls, (x.encoder if cls is not _DenseLoader and eng._loss_names else None)


def loader_for(eng, x, y=None):
    """The loader that fills `eng`'s buffers from this batch: picked by the kind of batch and kept in `eng.loaders`; a compact or
    resident batch with a new encoder object gets a new loader."""
    cls, enc = _pick(eng, x)
    ld = eng.loaders.get(cls)
    if ld is None or ld.enc is not enc:
        ld = eng.loaders[cls] = cls(eng, enc)
    return ld


def loader_ahead(eng, ran, x, y=None):
    """fit's look-ahead: the loader that may stage this NEXT batch while the step that loader `ran` filled is on the GPU, or None.
    A dense batch needs its targets and host arrays, whatever ran; a compact batch the very loader that ran (same encoder
    object: nothing is built under the step); a resident batch has nothing to upload."""
    cls, enc = _pick(eng, x)
    if cls is _DenseLoader:
        return loader_for(eng, x, y) if y is not None and not isinstance(x, H.DeviceBuffer) else None
    return ran if cls.stages_ahead and type(ran) is cls and ran.enc is enc else None
