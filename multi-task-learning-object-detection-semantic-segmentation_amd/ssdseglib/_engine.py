"""`Engine`: a `_graph.Model` lowered to a static list of the fused HIP launches of `_ops` (forward list, reversed backward list)
for a fixed batch size and mode -- the stand-in for Keras' GradientTape and Adam (third-party).
Everything stays resident in HBM (288 GB): no recomputation, no activation re-use planning; the launch list is static (no
Python-side decisions inside a step besides the op order).  The engine owns the parameter buckets and forward / backward over
the op list, and holds what construction leaves behind: `_lowering.Lowering` builds `ops`, `stores`, `vals`, `loss_ops` and
`input_store` (the concat plan and every fusion decision are its own), `_branches.plan_branches` splits the ops between the two
streams (`_schedule` gates and caches it).  `_loss_bind` binds the compiled losses and metrics to the engine, `_loaders` fills
its input and target buffers; fit / predict / evaluate are `_fit`.  The optimizer is `_optim.OptimState`, one per parameter set
(`engine.opt`): its state and every update launch live there, and `optimizer_step` / `adam_step` below only delegate.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _graph as K
from . import _hip as H
from ._branches import DET_OUTPUTS, plan_branches
from ._loss_bind import LossBinding, bind_losses, bind_metrics, launch_metrics  # noqa: F401  (LossBinding: re-exported)
from ._lowering import Lowering
from ._optim import OptimState
from ._ops import ACT_NONE, Op, Store, Val, pad4
from ._ops import BilinearOp, Conv3Op, DecodeNmsOp  # noqa: F401  (re-exported: tests name them through this module, as they did)


# ====================================================================================================== engine
class Engine:
    """One lowered instance of a model for a fixed batch size and mode."""

    def __init__(self, model: K.Model, batch_size: int, training: bool, ctx: Optional[H.Context] = None, grad_bucket=None):
        self.model, self.batch, self.training = model, int(batch_size), bool(training)
        self.ctx = ctx if ctx is not None else default_context()
        self.ops: List[Op] = []
        self.vals: Dict[int, Val] = {}          # id(KTensor) -> Val
        self.stores: List[Store] = []
        self.output_vals: List[Val] = []
        self.loss_ops: Dict[str, Op] = {}
        self._wt_rows: List[Tuple[int, int, int, int]] = []
        self._wt_table = None
        self._loss_names, self._metrics = [], []    # _loss_bind: LossBinding; (key, kind, fn, op, buffer)
        self._plans = None                          # _schedule's (trunk, detection, mask, join_before), dropped by _emit
        self._padded, self._padded_tables = {}, {}  # _padded_view / _sync_padded: zero-padded copies of odd-width weights
        self.loaders: dict = {}                     # _loaders.loader_for: loader class -> what fills this engine's buffers
        self.eval_stager = None                     # _fit.run_evaluate
        self._alloc_params(grad_bucket)
        Lowering(self).run()                        # -> ops, stores, vals, loss_ops, input_store
        self.output_vals = [self.vals[id(t)] for t in model.outputs]

    # ------------------------------------------------------------------ parameters
    def _alloc_params(self, grad_bucket):
        holder = getattr(self.model, "_trained", None) or self.model   # an inference model shares its trained model's weights
        owner = getattr(holder, "_engine_params", None)
        if owner is None:
            tr, st = [], []
            for l in self.model.layers:
                for wname, arr in l.weights.items():
                    (tr if (wname in l.trainable_names) else st).append((l, wname, arr))
            n_tr = sum(a.size for _, _, a in tr)
            n_st = sum(a.size for _, _, a in st)
            ctx = self.ctx
            owner = dict(index={}, n_tr=n_tr, n_st=n_st)
            flat = np.concatenate([a.reshape(-1) for _, _, a in tr]) if tr else np.zeros(0, np.float32)
            flat_s = np.concatenate([a.reshape(-1) for _, _, a in st]) if st else np.zeros(0, np.float32)
            owner["params"] = ctx.array(flat.astype(np.float32))
            owner["state"] = ctx.array(flat_s.astype(np.float32))
            off = 0
            for l, wname, arr in tr:
                owner["index"][(id(l), wname)] = ("params", off, arr.shape)
                off += arr.size
            off = 0
            for l, wname, arr in st:
                owner["index"][(id(l), wname)] = ("state", off, arr.shape)
                off += arr.size
            owner["grads"] = None
            owner["opt"] = holder._optim = OptimState(owner, holder)
            holder._engine_params = owner
            for l in self.model.layers:
                if l.weights:
                    l._engine_sync = (self._pull_layer, self._push_layer)
        self.P, self.opt = owner, owner["opt"]
        if self.training and owner["grads"] is None:
            owner["grads"] = grad_bucket if grad_bucket is not None else self.ctx.zeros(owner["n_tr"])
            # Adam's two buckets, also under SGD: dropping them there would change the order of device allocations under every
            # benchmark, which is a change of its own
            self.opt.slot("m"), self.opt.slot("v")

    @staticmethod
    def _phys_shape(wname: str, shape) -> Tuple[int, ...]:
        """shape of a weight as the kernels see it: channel dimensions rounded up to multiples of 4 (only ShuffleNetV2 '1x' /
        '2x' have any that are not: 58 / 122); taps, the 3 image channels and depth multipliers stay"""
        s = tuple(int(x) for x in shape)
        if len(s) == 1:                                     # BatchNormalization vectors, biases
            return (pad4(s[0]),)
        if wname == "depthwise_kernel":                     # (kh, kw, c, 1)
            return (s[0], s[1], pad4(s[2]), s[3])
        if len(s) == 4 and s[0] == 1 and s[1] == 1:         # pointwise kernels (1, 1, cin, cout)
            return (1, 1, pad4(s[2]), pad4(s[3]))
        return s

    def _bucket_view(self, layer, wname, grads=False):
        which, off, shape = self.P["index"][(id(layer), wname)]
        return (self.P["grads"] if grads else self.P[which]).view(off, shape)

    def _padded_view(self, layer, wname, kind: str):
        """zero-padded device copy of a weight (kind "p": parameter / state, refreshed from the bucket before every forward pass;
        "g": gradient, folded back into the bucket after the backward pass)"""
        which, off, shape = self.P["index"][(id(layer), wname)]
        phys = self._phys_shape(wname, shape)
        reg = self._padded
        key = (id(layer), wname, kind)
        if key not in reg:
            dims = [d for d in shape if d != 1] or [1]
            pdims = [d for d in phys if d != 1] or [1]
            rows = int(np.prod(dims[:-1])) if len(dims) > 1 else 1
            reg[key] = dict(buf=self.ctx.zeros(phys), rows=rows, cols=dims[-1], lds=dims[-1], ldd=pdims[-1], layer=layer, wname=wname,
                            which=which)
        return reg[key]["buf"]

    def register_wt(self, w: H.DeviceBuffer, m: int, ldx: int, k: int, n: int):
        """device buffer for the transposed copy Wt[n][k] of a pointwise kernel, refreshed by `_refresh_wt` at the start of every
        forward pass (None where the library's default dispatch for this shape does not stream a transposed copy)"""
        if self.ctx.parts("ssdseg_pwconv_wt_floats", m, ldx, k, n) == 0:
            return None
        wt = self.ctx.empty((n, k))
        self._wt_rows.append((w.ptr, wt.ptr, k, n))
        self._wt_table = None
        return wt

    def _refresh_wt(self):
        if not self._wt_rows:
            return
        if self._wt_table is None:
            self._wt_table = self.ctx.array(np.asarray(self._wt_rows, dtype=np.int64))
        tiles = max(-(-k // 32) * -(-n // 32) for _, _, k, n in self._wt_rows)
        self.ctx.call("ssdseg_transpose_batch", self._wt_table, len(self._wt_rows), tiles, sum(k * n for _, _, k, n in self._wt_rows))

    def param_view(self, layer, wname):
        which, off, shape = self.P["index"][(id(layer), wname)]
        if self._phys_shape(wname, shape) != tuple(shape):
            return self._padded_view(layer, wname, "p")
        return self.P[which].view(off, shape)

    state_view = param_view

    def grad_view(self, layer, wname):
        if not self.training:
            return None
        which, off, shape = self.P["index"][(id(layer), wname)]
        assert which == "params"
        if self._phys_shape(wname, shape) != tuple(shape):
            return self._padded_view(layer, wname, "g")
        return self.P["grads"].view(off, shape)

    def grad_array(self, layer, wname) -> np.ndarray:
        """this step's gradient of a weight in its Keras shape (tests)"""
        return self._bucket_view(layer, wname, grads=True).download()

    def _sync_padded(self, kind: str, to_bucket: bool, which: Optional[str] = None):
        """zero-padded copies of odd-width weights <-> their Keras-shaped slots of the flat bucket: ONE table-driven launch per call
        (ssdseg_copy2d_batch; the table is built once per (kind, direction, which) -- the pointers never change).  Was one
        ssdseg_copy2d per tensor: 160 launches per ShuffleNetV2-1x step (SSDSEG_COPY2D_BATCH=0 keeps that, bit-identical)."""
        padded = self._padded
        if not padded:
            return
        key = (kind, to_bucket, which, len(padded))            # (a table made before the last padded tensor was registered is not reused)
        cache = self._padded_tables
        if key not in cache:
            rows = []
            for (lid, wname, k), r in padded.items():
                if k != kind or (which is not None and r["which"] != which):
                    continue
                bv = self._bucket_view(r["layer"], wname, grads=(kind == "g"))
                if to_bucket:
                    rows.append((bv.ptr, r["lds"], r["buf"].ptr, r["ldd"], r["rows"], r["cols"]))
                else:
                    rows.append((r["buf"].ptr, r["ldd"], bv.ptr, r["lds"], r["rows"], r["cols"]))
            cache[key] = (rows, self.ctx.array(np.asarray(rows, dtype=np.int64)) if rows else None)
        rows, table = cache[key]
        if not rows:
            return
        if os.environ.get("SSDSEG_COPY2D_BATCH", "1") == "0":
            for dst, ldd, src, lds, nr, nc in rows:
                self.ctx.call("ssdseg_copy2d", C.c_void_p(dst), ldd, C.c_void_p(src), lds, nr, nc)
            return
        self.ctx.call("ssdseg_copy2d_batch", table, len(rows), max(nr * nc for *_, nr, nc in rows), sum(nr * nc for *_, nr, nc in rows))

    def _pull_layer(self, layer):
        self.ctx.sync()
        for wname in layer.weights:
            layer.weights[wname] = self._bucket_view(layer, wname).download()

    def _push_layer(self, layer):
        for wname, arr in layer.weights.items():
            self._bucket_view(layer, wname).upload(arr)

    # ------------------------------------------------------------------ ops added after construction, the branch schedule
    DET_OUTPUTS = DET_OUTPUTS
    keep_mask_probabilities = False         # a training engine's mask head also stores its probabilities (tests read them)
    _cur_reach = frozenset()                # the reach `_emit` gives an op: `_loss_bind` sets it for the detection loss op

    def _emit(self, op: Op):
        """an op that joins the list after the lowering (`_loss_bind._det_op`)"""
        op.reach = self._cur_reach
        self.ops.append(op)
        self._plans = None
        return op

    def _schedule(self):
        """-> (trunk, detection, mask, join_before) of `_branches.plan_branches` for a training engine, else everything in layer
        order on one stream"""
        if not self.training or os.environ.get("SSDSEG_DET_SIDE", "1") == "0":      # (read per pass: A/B runs and tests flip it)
            return self.ops, [], [], set()
        if self._plans is None:
            self._plans = plan_branches(self.ops, self.DET_OUTPUTS)
        return self._plans

    # ------------------------------------------------------------------ execution
    def set_input(self, images):
        if isinstance(images, H.DeviceBuffer):
            if images.ptr != self.input_store.buf.ptr:
                self.input_store.buf.copy_from(images)
        else:
            a = np.ascontiguousarray(images, dtype=np.float32)
            assert a.shape == (self.batch, self.input_store.h, self.input_store.w, self.input_store.c), f"input shape {a.shape}"
            self.input_store.buf.upload(a)

    def forward(self):
        trunk, det, mask, _ = self._schedule()
        if det:
            # a training forward leaves the detection branch running on the side stream; a second forward() before backward()
            # (which joins) would overwrite the trunk activations and weight copies it may still read (no-op after a whole step)
            self.ctx.join()
        self._sync_padded("p", to_bucket=False)          # padded copies of the weights <- bucket (no-op for most models)
        self._refresh_wt()                                # transposed copies of the pointwise kernels: one launch
        for op in trunk:
            op.fwd()
        if det:
            self.ctx.side(True)              # forks behind the trunk: the detection branch runs beside the mask branch
            for op in det:
                op.fwd()
            self.ctx.side(False)
            for op in mask:
                op.fwd()
            if self._metrics:
                self.ctx.join()              # the metric kernels read both branches' outputs on the main stream
        if self.training:
            self._sync_padded("p", to_bucket=True, which="state")   # moving statistics of padded BatchNorms -> bucket

    def _begin_backward(self):
        """no gradient is written yet; the column sums that fold the weight-gradient partial slabs are recorded during the pass and
        launched ONCE by the join at its end (include/ssdseg.h: ssdseg_colsum_defer); SSDSEG_COLSUM_DEFER=0 keeps one launch per
        layer (A/B runs, bit-identical results)"""
        self.ctx.colsum_defer(os.environ.get("SSDSEG_COLSUM_DEFER", "1") != "0")
        for s in self.stores:
            s.gwritten = False

    def _end_backward(self):
        for s in self.stores:
            s._materialise_pending()
        self.ctx.join()     # weight-gradient kernels on the side stream: done before anyone (optimizer, all-reduce) reads them
        self._sync_padded("g", to_bucket=True)   # gradients of zero-padded weights -> their Keras-shaped slots of the bucket
        self.ctx.colsum_defer(False)   # deferral ends with the pass: a later entry point on this context folds its slabs at once

    def backward(self):
        self._begin_backward()
        for s in self.stores:
            if s.split_parent and s.need_grad:
                s.grad.zero_()
                s.gwritten = True
        trunk, det, mask, join_before = self._schedule()
        if det:
            self.ctx.side(True)
            for op in reversed(det):
                op.bwd()
            self.ctx.side(False)
            # the main stream has to wait for the END OF THE DETECTION BRANCH twice -- not for the side stream as a whole, which by
            # then also carries the mask branch's weight gradients, queued behind it (a join there stalled the main stream for them)
            wait = self.ctx.join if os.environ.get("SSDSEG_DET_SIDE") == "join" else self.ctx.side_wait_mark      # (A/B: full joins)
            self.ctx.side_mark()
            for op in reversed(mask):
                if id(op) in join_before:
                    wait()                         # this op adds to a gradient the detection branch wrote first
                    join_before = ()
                op.bwd()
            wait()                                 # the trunk's backward reads both branches' gradients
        for op in reversed(trunk):
            op.bwd()
        self._end_backward()

    def seed_output_grad(self, index: int, g):
        """inject dL/d(output[index]) (bench config 2 / tests): output values are the ACTIVATED tensors"""
        v = self.output_vals[index]
        buf = v.store.grad
        if isinstance(g, H.DeviceBuffer):
            buf.copy_from(g)
        else:
            buf.upload(np.ascontiguousarray(g, np.float32))

    def mark_output_grads_written(self):
        for v in self.output_vals:
            v.store.gwritten = True

    def backward_from_outputs(self):
        self._begin_backward()
        self.mark_output_grads_written()
        for op in reversed(self.ops):
            op.bwd()
        self._end_backward()

    def output(self, index: int) -> np.ndarray:
        """activated value of output `index` as a NumPy array (N, H, W, C) -- for tests / predict"""
        v = self.output_vals[index]
        s = v.store
        if v.scale is None and v.act == ACT_NONE and s.ld == s.c:
            arr = s.buf.download().reshape(s.n, s.h, s.w, s.ld)
        else:
            tmp = self.ctx.empty((s.m, s.c))
            self.ctx.call("ssdseg_bn_apply", v.view(), s.ld, None, 0, tmp, s.c, s.m, s.c)
            arr = tmp.download().reshape(s.n, s.h, s.w, s.c)
        shp = self.model.outputs[index].shape
        if arr.shape[-1] != shp[-1] and arr.ndim == 4 and len(shp) == 4:
            arr = np.ascontiguousarray(arr[..., :shp[-1]])      # zero-padded channels of an odd-width tensor
        return arr.reshape((s.n,) + tuple(shp[1:]))

    # ------------------------------------------------------------------ training step (Keras train_step stand-in)
    def configure_losses(self, loss: dict, loss_weights: dict):
        bind_losses(self, loss, loss_weights)

    def configure_metrics(self, metrics: dict):
        bind_metrics(self, metrics)

    def compute_metrics(self):
        launch_metrics(self)

    def set_targets(self, targets: dict):
        for r in self._loss_names:
            y, dst = targets[r.name], r.target
            if isinstance(y, H.DeviceBuffer):
                if y.ptr != dst.ptr:
                    dst.copy_from(y)
            else:
                dst.upload(np.ascontiguousarray(y, np.float32))

    def losses(self) -> Dict[str, float]:
        """batch means of the per-sample losses, Keras naming (`loss`, `<output>_loss`)"""
        out, total = {}, 0.0
        for r in self._loss_names:
            v = float(r.loss.download().mean())
            out[f"{r.name}_loss"] = v
            total += r.weight * v
        out["loss"] = total
        for key, kind, fn, op, buf in self._metrics:
            out[key] = float(buf.download().mean())        # batch mean, NaN-propagating like Keras (quirk Q10)
        return out

    def train_step(self, images=None, targets=None, optimizer=None, allreduce=None, world=1):
        self.opt.check_not_averaging()
        if images is not None:
            self.set_input(images)
        if targets is not None:
            self.set_targets(targets)
        self.forward()
        self.compute_metrics()
        self.backward()
        if allreduce is not None:
            allreduce()
        self.optimizer_step(optimizer, grad_scale=1.0 / world)

    def optimizer_step(self, o, grad_scale=1.0):
        self.opt.step_with(o, grad_scale)

    def adam_step(self, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, decay=None, clip=None):
        self.opt.adam(lr, beta1, beta2, eps, grad_scale, decay, clip)


_default_ctx: Optional[H.Context] = None


def default_context() -> H.Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = H.Context(0)
    return _default_ctx


def set_default_context(ctx: H.Context):
    global _default_ctx
    _default_ctx = ctx


def engine_for(model: K.Model, batch_size: int, training: bool, mode=None) -> Engine:
    """the model's engine for this batch size and mode, built on first use; a training engine binds the compiled losses and metrics"""
    cache = model.__dict__.setdefault("_engines", {})
    key = (int(batch_size), mode or bool(training))
    if key not in cache:
        eng = Engine(model, batch_size, training)
        if training or mode == "eval":
            comp = model._compiled
            if comp is None:
                raise RuntimeError("call model.compile(optimizer=..., loss=...) before fit / train_on_batch")
            eng.configure_losses(comp["loss"], comp["loss_weights"])
            eng.configure_metrics(comp.get("metrics") or {})
        cache[key] = eng
    return cache[key]


def eval_engine_for(model: K.Model, batch_size: int) -> Engine:
    """inference-mode engine that also evaluates the compiled losses (validation_data of fit)"""
    return engine_for(model, batch_size, False, mode="eval")

