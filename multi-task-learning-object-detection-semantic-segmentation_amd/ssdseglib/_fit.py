"""The Keras-like entry points over `_engine.Engine` and `_loaders`, called by `_graph.Model` and `evaluators`: forward / predict,
evaluate on the device, train_on_batch, fit.  Engines are looked up as attributes of `_engine` at call time.
"""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np

from . import _engine as E
from . import _graph as K
from ._loaders import _DenseLoader, _ResidentLoader, batch_size, loader_ahead, loader_for
from ._ops import DecodeNmsOp


def _postprocess(model: K.Model, eng: E.Engine, index: int) -> np.ndarray:
    out = eng.output(index)
    nms = eng.output_vals[index].meta.get("nms")
    if nms is not None and nms.suppress_background_boxes:
        out = out.reshape(-1, 6)        # quirk Q7 (reference layers.py:165-166): boolean_mask drops the batch axis
        out = out[out[:, 0] > 0]
    return out


def run_forward(model: K.Model, x, training: bool = False) -> List[np.ndarray]:
    """model(x, training=False) -> list of output arrays (NB03#cell31)"""
    x = np.asarray(x, np.float32)
    if x.ndim == 3:
        x = x[None]
    eng = E.engine_for(model, x.shape[0], False)
    eng.set_input(x)
    eng.forward()
    return [_postprocess(model, eng, i) for i in range(len(model.outputs))]


def _batches(data):
    """accepts an iterable of batches: x, (x,), (x, y) with y a dict keyed by output name"""
    for item in data:
        if isinstance(item, (tuple, list)):
            yield item[0], (item[1] if len(item) > 1 else None)
        else:
            yield item, None


def run_predict(model: K.Model, data) -> List[np.ndarray]:
    """model.predict(dataset) -> outputs concatenated over the batches (NB03#cell25)"""
    if isinstance(data, np.ndarray):
        data = [data[i:i + 16] for i in range(0, data.shape[0], 16)]
    chunks = [run_forward(model, x) for x, _ in _batches(data)]
    return [np.concatenate([c[i] for c in chunks], axis=0) for i in range(len(model.outputs))]


class _EvalStager:
    """A test batch (`datacoder.CompactBatch` or `ResidentBatch`, un-augmented) into an inference engine, and the engine's outputs
    into the numbers of NB03#cell21-29 without leaving the device: the batch's loader (no encoder, no targets) fills the engine's
    input and its own gt / cnt; the uint8 class indices go to ssdseg_eval_mask_jaccard as they are, the ground-truth rows to
    ssdseg_eval_det_best_iou.  Per batch: iou (n, c), and per NMS threshold pair the detection rows (n, r, 6) and their best IoU (n, r).
    With `ignore_void` or `confusion` the mask step is ssdseg_eval_mask_scores instead: the same single pass over the probabilities,
    which also leaves the per-image confusion counts (n, c, c) and void pixels (n,)."""

    def __init__(self, eng: E.Engine):
        self.eng, self.ctx = eng, eng.ctx
        ctx, b, ins = eng.ctx, eng.batch, eng.input_store
        v = eng.output_vals[0]
        if "mask_head" not in v.meta or v.store.ld != v.store.c:
            raise ValueError("evaluate_on_device needs a model from get_model_for_inference (outputs: mask probabilities, detections)")
        self.prob = v.store
        self.nms_op = next((op for op in eng.ops if isinstance(op, DecodeNmsOp)), None)
        if self.nms_op is None:
            raise ValueError("evaluate_on_device needs a model from get_model_for_inference (no NMS layer in this one)")
        self.r = self.nms_op.out.h
        self.midx = ctx.empty((b, ins.h, ins.w), np.uint8)      # class indices of a resident batch whose slots are scattered
        self.det = ctx.empty((b, self.r, 6))
        self.best = ctx.empty((b, self.r))
        self.iou = ctx.empty((b, self.prob.c))
        self.confusion = self.void = None                       # allocated by the first call that asks for the confusion counts

    def load(self, batch):
        """the batch through its loader (pixels -> the engine's input, ground truth -> ld.gt / ld.cnt) -> (ld, its class indices [b][hw])"""
        b, ins = self.eng.batch, self.eng.input_store
        if batch.augmented_by():      # (the class indices returned below are as the files hold them)
            raise ValueError("evaluate_on_device: the batch carries crop windows, a mosaic, colour draws or flip flags; a test set is not augmented")
        ld = loader_for(self.eng, batch)
        ld.stage(batch)
        ld.consume()
        if not isinstance(ld, _ResidentLoader):
            return ld, ld.midx
        ds, hw, first = batch.dataset, ins.h * ins.w, int(batch.index[0])
        if np.array_equal(batch.index, np.arange(first, first + b)):
            return ld, ds.masks.view(first * hw, (b, hw))             # consecutive slots: the pool itself
        for i, s in enumerate(batch.index):
            self.midx.view(i * hw, (hw,)).copy_from(ds.masks.view(int(s) * hw, (hw,)))
        return ld, self.midx

    def run(self, batch, pairs, ignore_void=False, confusion=False):
        """-> iou (n, c) float32, {pair: (detections (n, r, 6), best IoU (n, r))}, counts: one network forward, one decode (+
        segmentation suppression), then per threshold pair (or triple with a Soft-NMS sigma; a pair runs the layer's own) the NMS
        and the best-IoU kernel.  counts: None, or with `confusion`
        (confusion (n, c, c), void pixels (n,)) as int32"""
        eng, ctx, op, b = self.eng, self.ctx, self.nms_op, self.eng.batch
        ld, midx = self.load(batch)
        op.defer_nms = True
        try:
            eng.forward()
        finally:
            op.defer_nms = False
        counts = None
        if not (ignore_void or confusion):
            ctx.call("ssdseg_eval_mask_jaccard", self.prob.buf, midx, b, self.prob.h * self.prob.w, self.prob.c, self.iou)
        else:
            if confusion and self.confusion is None:
                self.confusion, self.void = ctx.empty((b, self.prob.c, self.prob.c), np.int32), ctx.empty(b, np.int32)
            ctx.call("ssdseg_eval_mask_scores", self.prob.buf, midx, b, self.prob.h * self.prob.w, self.prob.c, int(ignore_void), self.iou,
                     self.confusion if confusion else None, self.void if confusion else None)
            if confusion:
                counts = (self.confusion.download(), self.void.download())
        iou = self.iou.download()
        out = {}
        for pair in pairs:
            op.run_nms(pair[0], pair[1], pair[2] if len(pair) > 2 else None, out=self.det)     # (b_thr, p_thr[, Soft-NMS sigma])
            ctx.call("ssdseg_eval_det_best_iou", self.det, ld.gt, ld.cnt, b, self.r, ld.GMAX, self.best)
            out[pair] = (self.det.download(), self.best.download())
        return iou, out, counts


def _eval_stager(model: K.Model, batch) -> _EvalStager:
    eng = E.engine_for(model, len(batch), False)
    if eng.eval_stager is None:
        eng.eval_stager = _EvalStager(eng)
    return eng.eval_stager


def run_evaluate(model: K.Model, batch, pairs):
    """evaluators.evaluate_on_device's device side for one batch: (iou, {pair: (detections, best IoU)}), see _EvalStager.run.  A
    batch of another size gets an engine of its own, as in predict."""
    return _eval_stager(model, batch).run(batch, pairs)[:2]


def run_evaluate_scores(model: K.Model, batch, pairs, ignore_void: bool, confusion: bool):
    """run_evaluate with evaluate_on_device's mask options: (iou, {pair: ...}, None | (confusion (n, c, c), void pixels (n,)))"""
    return _eval_stager(model, batch).run(batch, pairs, ignore_void, confusion)


def run_train_on_batch(model: K.Model, x, y=None) -> Dict[str, float]:
    eng = E.engine_for(model, batch_size(x), True)
    ld = loader_for(eng, x, y)
    ld.stage(x, y)
    ld.consume()
    eng.train_step(optimizer=model._compiled.get("optimizer"))
    return eng.losses()


class History:
    def __init__(self):
        self.history: Dict[str, List[float]] = {}
        self.epoch: List[int] = []


def run_fit(model: K.Model, data, epochs=1, validation_data=None, verbose=0) -> History:
    """model.fit(ds, epochs, validation_data, verbose) (NB03#cell16): the last partial batch is kept (its own batch
    statistics and mining pool); per-epoch means weighted by batch size, Keras history keys."""
    hist = History()
    overlap = os.environ.get("SSDSEG_FIT_OVERLAP", "1") != "0"
    for epoch in range(epochs):
        sums, seen = {}, 0
        it = iter(_batches(data))
        cur = next(it, None)
        staged = None          # the batch whose upload is in flight
        while cur is not None:
            n = batch_size(cur[0])
            eng = E.engine_for(model, n, True)
            ld = loader_for(eng, *cur)
            if staged is not cur:
                ld.stage(*cur)
            ld.consume()                            # compact / resident: expansion + anchor encoding on the device
            eng.train_step(optimizer=model._compiled.get("optimizer"))
            # the step is queued; everything below runs on the host while the GPU works on it
            nxt = next(it, None)
            ahead = loader_ahead(eng, ld, *nxt) if overlap and nxt is not None and batch_size(nxt[0]) == n else None
            staged = nxt if ahead is not None and ahead.stage(*nxt, ahead=True) else None     # on the copy stream, under the step just queued
            for k, v in eng.losses().items():
                sums[k] = sums.get(k, 0.0) + v * n
            seen += n
            cur = nxt
        logs = {k: v / max(seen, 1) for k, v in sums.items()}
        opt = model._compiled.get("optimizer")
        if seen and opt is not None and callable(getattr(opt, "learning_rate", None)):
            logs["lr"] = float(np.float32(eng.opt.lr))      # a scheduled rate: the one of the epoch's last step, as the kernel took it
        if seen and getattr(opt, "global_clipnorm", None) is not None:
            logs["grad_norm"] = float(eng.opt.clip.download()[0])      # the pre-clip norm of the epoch's last update: 8 bytes, once per epoch
        if validation_data is not None:
            vs, vseen = {}, 0
            for x, y in _batches(validation_data):
                n = batch_size(x)
                eng = E.eval_engine_for(model, n)      # moving statistics, no gradient buffers (Keras test_step)
                ld = loader_for(eng, x, y)
                if y is None and isinstance(ld, _DenseLoader):
                    raise ValueError("validation_data: a batch of dense arrays needs its targets, (x, y)")
                ld.stage(x, y)
                ld.consume()
                eng.forward()
                eng.compute_metrics()
                for k, v in eng.losses().items():
                    vs[k] = vs.get(k, 0.0) + v * n
                vseen += n
            logs.update({f"val_{k}": v / max(vseen, 1) for k, v in vs.items()})
        for k, v in logs.items():
            hist.history.setdefault(k, []).append(v)
        hist.epoch.append(epoch)
        if verbose:
            print(f"Epoch {epoch + 1}/{epochs} - " + " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()))
    return hist
