"""`Engine`: a `_graph.Model` lowered to a static list of the fused HIP launches of `_ops` (forward list, reversed backward list)
for a fixed batch size and mode -- the stand-in for Keras' GradientTape and Adam (third-party).
Everything stays resident in HBM (288 GB): no recomputation, no activation re-use planning; the launch list is static (no
Python-side decisions inside a step besides the op order).  The engine owns the parameter bucket, the concat plan, the
two-stream schedule, the lowering and forward / backward.  `_loss_bind` binds the compiled losses and metrics to it, `_loaders` fills
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
from . import layers as L
from ._loss_bind import LossBinding, bind_losses, bind_metrics, launch_metrics  # noqa: F401  (LossBinding: re-exported)
from ._optim import OptimState
from ._ops import (ACT_NONE, ACT_RELU, ActBwdOp, ApplyOp, BilinearOp, BNRec, BnOp, ChannelStatsOp, Conv3Op, DecodeNmsOp, DwOp, GapOp,
                   HeadGatherOp, MaskHeadOp, MaxPoolOp, Op, PwOp, ShuffleOp, SoftmaxRowsOp, SplitGatherOp, StemOp, Store, TableShuffleOp,
                   Val, _act_of, _nonneg, pad4)


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
        self._plan_concats()
        reach = self._outputs_reached()
        self._cur_reach = frozenset()
        for layer in model.layers:
            self._cur_reach = reach[id(layer)]
            self._lower(layer)
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

    # ------------------------------------------------------------------ planning helpers
    def _plan_concats(self):
        """channel-axis Concatenate: let each input's storage producer write straight into its slice"""
        self.cons: Dict[int, List[K.Layer]] = {}                    # id(tensor) -> the layers that read it
        for l in self.model.layers:
            for t in l.inbound:
                self.cons.setdefault(id(t), []).append(l)
        self.placement: Dict[int, Tuple[K.Concatenate, int]] = {}   # id(producer layer) -> (concat layer, channel offset)
        self.concat_store: Dict[int, Store] = {}
        outs = {id(t) for t in self.model.outputs}
        for l in self.model.layers:
            if not isinstance(l, K.Concatenate) or l.axis_resolved != 3:
                continue
            off = 0
            for t in l.inbound:
                c = pad4(t.shape[-1])
                cur, ok = t, True
                # walk back through lazily-fused per-channel layers to whoever writes memory
                while isinstance(cur.layer, (K.ReLU, K.BatchNormalization)):
                    if len(self.cons.get(id(cur), [])) != 1 or id(cur) in outs:
                        ok = False
                        break
                    cur = cur.layer.inbound[0]
                prod = cur.layer
                if ok and isinstance(prod, (K.Conv2D, K.SeparableConv2D, K.UpSampling2D)) and len(self.cons.get(id(cur), [])) == 1 \
                        and id(cur) not in outs and not (isinstance(prod, K.Conv2D) and prod.kernel_size == (3, 3)):
                    self.placement[id(prod)] = (l, off)
                off += c

    def _concat_parts(self, concat: K.Concatenate):
        """(store, wide scale, wide shift) of a channel concat, created on first use"""
        key = id(concat)
        if key not in self.concat_store:
            n, h, w, _ = (self.batch,) + tuple(concat.outputs[0].shape[1:])
            parts, c = [], 0                       # physical layout: every input at its padded width
            for t in concat.inbound:
                parts.append((c, int(t.shape[-1])))
                c += pad4(t.shape[-1])
            st = Store(self, n, h, w, c, concat.name)
            st.logical_parts = parts
            st.wide_scale = self.ctx.array(np.ones(c, np.float32))
            st.wide_shift = self.ctx.array(np.zeros(c, np.float32))
            self.concat_store[key] = st
            self.stores.append(st)
        return self.concat_store[key]

    def _out_store(self, layer, shape, name=None) -> Tuple[Store, Optional[H.DeviceBuffer], Optional[H.DeviceBuffer]]:
        """fresh dense store for a layer's raw output, or its slice of a concat buffer"""
        n, h, w, c = (self.batch,) + tuple(shape[1:])
        c = pad4(c)                                # (== c for every model but ShuffleNetV2 '1x' / '2x')
        if id(layer) in self.placement:
            concat, off = self.placement[id(layer)]
            parent = self._concat_parts(concat)
            st = parent.slice(off, c, name or layer.name)
            st.slice_scale = parent.wide_scale.view(off, (c,))
            st.slice_shift = parent.wide_shift.view(off, (c,))
            return st
        st = Store(self, n, h, w, c, name or layer.name)
        self.stores.append(st)
        return st

    def _emit(self, op: Op):
        op.reach = self._cur_reach          # names of the model outputs that depend on this op (branch scheduling, _schedule)
        self.ops.append(op)
        self._plans = None
        return op

    # ------------------------------------------------------------------ two independent branches on two streams
    DET_OUTPUTS = frozenset(("output-labels", "output-boxes"))      # the reference's output names (models.py:259,271)

    def _outputs_reached(self) -> Dict[int, frozenset]:
        """id(layer) -> names of the model outputs that depend on it"""
        names = {id(t): t.layer.name for t in self.model.outputs}
        reach: Dict[int, frozenset] = {}
        for layer in reversed(self.model.layers):
            r = set()
            for t in layer.outputs:
                if id(t) in names:
                    r.add(names[id(t)])
                for c in self.cons.get(id(t), []):
                    r |= reach.get(id(c), frozenset())
            reach[id(layer)] = frozenset(r)
        return reach

    def _schedule(self):
        """The multi-task graph is a shared trunk with two independent branches.  Which is which follows from reachability, not
        from layer names: the mask output depends on the backbone only up to the block-13 expansion (ASPP tap) -- everything
        behind it (block 13's depthwise conv ... block 16, the extra feature maps, the eight SSDLite heads, gather, softmax,
        the detection losses: ~150 launches of 5-60 us on 30x40 ... 1x1 maps that leave most CUs idle) only feeds the detection
        outputs.  A training engine issues that DETECTION branch on the context's side stream -- forward right behind the
        trunk, backward right at the start -- so it runs beside the MASK branch (ASPP, decoder, mask head: few long kernels
        that fill the chip) instead of before / after it: 31.8 -> 30.5 ms per batch-32 step.  The backward issue order stays
        detection, mask, trunk = the reverse layer order for every tensor more than one of them touches (checked below), so every
        first-writer / accumulate decision and every summation order is the same and results are bit-identical with
        SSDSEG_DET_SIDE=0 (one stream, layer order).  Cross-stream hazards: a mask-branch backward op that accumulates into a
        trunk tensor's gradient the detection branch wrote first (the block-13 tap feeds the ASPP and the first SSD head) waits
        for the side stream (`join_before`); the trunk's backward joins anyway.
        -> (trunk, detection, mask, join_before)"""
        if not self.training or os.environ.get("SSDSEG_DET_SIDE", "1") == "0":      # (read per pass: A/B runs and tests flip it)
            return self.ops, [], [], set()
        if self._plans is not None:
            return self._plans
        def touched(op):
            out = set()
            for v in vars(op).values():
                for x in (v if isinstance(v, (list, tuple)) else (v,)):
                    st = x.store if isinstance(x, Val) else (x if isinstance(x, Store) else None)
                    while st is not None:
                        out.add(id(st))
                        st = st.parent
            return out

        pos = {id(op): i for i, op in enumerate(self.ops)}
        touch = {id(op): touched(op) for op in self.ops}
        det = [op for op in self.ops if op.reach and op.reach <= self.DET_OUTPUTS]
        mask = [op for op in self.ops if op.reach and not (op.reach & self.DET_OUTPUTS)]
        serial = (list(self.ops), [], [], set())
        if not det or not mask:
            self._plans = serial
            return self._plans
        # A detection-branch op that reads a tensor the mask branch also reads, and comes BEFORE those readers in layer order,
        # is the LAST to contribute to that tensor's gradient in the backward pass -- and may rely on it (the depthwise conv of
        # block 13 completes the block-13 tap's gradient and takes its BatchNorm's backward sums over the completed tensor,
        # DwOp.fuse_input_bn).  Such ops stay with the trunk: issued before the fork in the forward pass, after the join in the
        # backward pass, at their place in layer order.
        mask_last = {}
        for op in mask:
            for sid in touch[id(op)]:
                mask_last[sid] = max(mask_last.get(sid, -1), pos[id(op)])
        keep = [op for op in det if any(pos[id(op)] < mask_last.get(sid, -1) for sid in touch[id(op)])]
        det = [op for op in det if op not in keep]
        det_ids, mask_ids = {id(o) for o in det}, {id(o) for o in mask}
        trunk = [op for op in self.ops if id(op) not in det_ids and id(op) not in mask_ids]
        # Validity of the three-phase order (else: one stream, layer order).  (1) A demoted op runs before the fork, so nothing it
        # reads may come from the detection branch: no detection op ahead of it in layer order touches a tensor it touches.  (2) The backward
        # pass writes a tensor's gradient in the order detection, mask, trunk; that is the reverse layer order -- same first
        # writer, same accumulation order, bit-identical sums -- iff in layer order every trunk op on that tensor precedes every
        # branch op on it and every mask op precedes every detection op.
        det_out = set().union(*[touch[id(op)] for op in det]) if det else set()
        ok = bool(det) and not any(touch[id(k)] & touch[id(d)] for k in keep for d in det if pos[id(d)] < pos[id(k)])
        first = {}
        for kind, ops_ in (("det", det), ("mask", mask)):
            for op in ops_:
                for sid in touch[id(op)]:
                    f = first.setdefault(sid, {})
                    f[kind + "_min"] = min(f.get(kind + "_min", 1 << 30), pos[id(op)])
                    f[kind + "_max"] = max(f.get(kind + "_max", -1), pos[id(op)])
        for op in trunk:
            for sid in touch[id(op)] & set(first):
                f = first[sid]
                if pos[id(op)] > min(f.get("det_min", 1 << 30), f.get("mask_min", 1 << 30)):
                    ok = False
        for f in first.values():
            if "det_min" in f and "mask_max" in f and f["mask_max"] > f["det_min"]:
                ok = False
        if not ok:
            self._plans = serial
            return self._plans
        det_touch = det_out
        join_before = {id(op) for op in mask if touch[id(op)] & det_touch}
        self._plans = (trunk, det, mask, join_before)
        return self._plans

    def _dense(self, v: Val, name: str) -> Val:
        """a Val over a dense store (materialise sliced / strided inputs for kernels that need ld == c)"""
        if v.store.ld == v.store.c:
            return v
        s = v.store
        st = Store(self, s.n, s.h, s.w, s.c, name + ":dense")
        self.stores.append(st)
        self._emit(ApplyOp(self, v, None, st, name + ":dense"))
        return Val(st)

    # ------------------------------------------------------------------ lowering
    def _lower(self, layer: K.Layer):
        ins = [self.vals[id(t)] for t in layer.inbound]
        out_t = layer.outputs[0] if layer.outputs else None
        setv = lambda v: self.vals.__setitem__(id(out_t), v)

        if isinstance(layer, K.InputLayer):
            n, h, w, c = (self.batch,) + tuple(out_t.shape[1:])
            st = Store(self, n, h, w, c, layer.name, need_grad=False)
            self.stores.append(st)
            self.input_store = st
            setv(Val(st))
        elif isinstance(layer, K.Rescaling):
            setv(Val(ins[0].store, rescale=(layer.scale, layer.offset)))
        elif isinstance(layer, K.Conv2D):
            self._lower_conv(layer, ins[0], setv)
        elif isinstance(layer, K.DepthwiseConv2D):
            assert layer.strides[0] == layer.strides[1] and layer.dilation_rate[0] == layer.dilation_rate[1]
            st = self._out_store(layer, out_t.shape)
            op = self._emit(DwOp(self, layer, "depthwise_kernel", self._dense(ins[0], layer.name), st, layer.strides[0], layer.dilation_rate[0]))
            src = layer.inbound[0]
            cons = self.cons.get(id(src), [])
            op.fuse_input_bn = (op.inp is ins[0] and ins[0].bn is not None and ins[0].store.parent is None and bool(cons) and cons[0] is layer
                                and layer.dilation_rate[0] == 1)
            op.out_val = Val(st)
            setv(op.out_val)
            st.producer = op
        elif isinstance(layer, K.SeparableConv2D):
            assert layer.strides[0] == layer.strides[1] and layer.dilation_rate[0] == layer.dilation_rate[1]
            inp = self._dense(ins[0], layer.name)
            s = inp.store
            n, h, w, _ = (self.batch,) + tuple(out_t.shape[1:])
            mid = Store(self, n, h, w, s.c, layer.name + ":dw")
            self.stores.append(mid)
            dw = self._emit(DwOp(self, layer, "depthwise_kernel", inp, mid, layer.strides[0], layer.dilation_rate[0]))
            src = layer.inbound[0]
            # sole consumer of a BatchNorm(+ReLU) output (the decoder's sepconv behind the 3x3 conv): that BN's backward sums
            # ride in the depthwise backward, as for the MBConv blocks
            dw.fuse_input_bn = (inp is ins[0] and ins[0].bn is not None and ins[0].store.parent is None
                                and len(self.cons.get(id(src), [])) == 1 and id(src) not in {id(t) for t in self.model.outputs})
            mid.stats = None   # no BatchNormalization between the two halves
            dw.out_val = Val(mid)
            st = self._out_store(layer, out_t.shape)
            pw = self._emit(PwOp(self, layer, "pointwise_kernel", dw.out_val, st))
            pw.out_val = Val(st)
            st.producer = pw
            setv(pw.out_val)
        elif isinstance(layer, K.BatchNormalization):
            v = ins[0]
            assert v.scale is None and v.act == ACT_NONE and v.bn is None, f"{layer.name}: BatchNormalization input must be a raw conv output"
            st = v.store
            sc = getattr(st, "slice_scale", None)
            sh = getattr(st, "slice_shift", None)
            rec = BNRec(self, layer, st.c, sc, sh)
            if self.training and st.stats is None:
                self._emit(ChannelStatsOp(self, st))
            self._emit(BnOp(self, rec, st))
            nv = Val(st, rec.scale, rec.shift, ACT_NONE, rec)
            prod = getattr(st, "producer", None)
            if prod is not None:
                prod.out_val = nv
            setv(nv)
        elif isinstance(layer, K.ReLU):
            v = ins[0]
            act = _act_of(layer)
            assert v.act == ACT_NONE, f"{layer.name}: stacked activations are not used by ssdseglib"
            if v.bn is not None:
                assert len(self.cons.get(id(layer.inbound[0]), [])) == 1, f"{layer.name}: BN output feeds both a ReLU and another layer"
                v.bn.act = act
            elif act != ACT_NONE:
                # activation on a materialised tensor (ShuffleNetV2: ReLU after Add, models.py:593-595): consumers clamp on
                # load; in backward the gradient w.r.t. the activated value is masked in place before the producer runs
                assert len(self.cons.get(id(layer.inbound[0]), [])) == 1, f"{layer.name}: its input also feeds another layer"
                if self.training:
                    self._emit(ActBwdOp(self, v.store, act, layer.name))
            nv = Val(v.store, v.scale, v.shift, act, v.bn)
            prod = getattr(v.store, "producer", None)
            if prod is not None and v.bn is not None:
                prod.out_val = nv
            setv(nv)
        elif isinstance(layer, K.Add):
            st = self._out_store(layer, out_t.shape)
            op = self._emit(ApplyOp(self, ins[1], ins[0], st, layer.name))
            a = ins[1]
            if (self.training and a.bn is not None and a.store.parent is None and st.parent is None and a.store.ld == st.ld and a.store.c == st.c
                    and len(self.cons.get(id(layer.inbound[1]), [])) == 1 and id(layer.inbound[1]) not in {id(t) for t in self.model.outputs}):
                a.store._grad = st._raw_grad()    # dL/d(projection output) == dL/d(Add output): one buffer
                op.alias_a = True
            setv(Val(st))
        elif isinstance(layer, K.Concatenate):
            self._lower_concat(layer, ins, setv)
        elif isinstance(layer, K.GlobalAveragePooling2D):
            st = self._out_store(layer, out_t.shape)
            self._emit(GapOp(self, self._dense(ins[0], layer.name), st, layer.name))
            setv(Val(st))
        elif isinstance(layer, K.UpSampling2D):
            cons = self.cons.get(id(out_t), [])
            if len(cons) == 1 and isinstance(cons[0], K.Softmax):
                setv(Val(ins[0].store, ins[0].scale, ins[0].shift, ins[0].act, ins[0].bn, lazy_up=layer.size, src=ins[0]))
            else:
                st = self._out_store(layer, out_t.shape)
                self._emit(BilinearOp(self, ins[0], st, layer.size[0], layer.size[1], layer.name))
                # values are already activated; the concat-wide activation is idempotent on them
                setv(Val(st, materialised_act=ins[0].act))
        elif isinstance(layer, K.Softmax):
            self._lower_softmax(layer, ins[0], setv)
        elif isinstance(layer, K.Reshape):
            self._lower_reshape(layer, ins[0], setv)
        elif isinstance(layer, L.DecodeBoxesCentroidsOffsets):
            setv(Val(ins[0].store, decode=layer))
        elif isinstance(layer, L.SegmentationSuppression):
            setv(Val(ins[1].store, suppress_with=ins[0].store))
        elif isinstance(layer, L.NonMaximumSuppression):
            boxes_v, probs_v = ins[0], ins[1]
            out = Store(self, self.batch, layer.max_number_of_boxes_per_sample, 1, 6, layer.name, need_grad=False)
            self.stores.append(out)
            self._emit(DecodeNmsOp(self, boxes_v.store, probs_v.store, boxes_v.meta["decode"], layer, probs_v.meta.get("suppress_with"), out))
            setv(Val(out, nms=layer))
        else:
            self._lower_shufflenet(layer, ins, setv)

    def _lower_conv(self, layer: K.Conv2D, v: Val, setv):
        out_t = layer.outputs[0]
        if "rescale" in v.meta:
            assert layer.kernel_size == (3, 3) and layer.strides == (2, 2), "Rescaling must feed the 3x3 stride-2 stem"
            st = self._out_store(layer, out_t.shape)
            op = self._emit(StemOp(self, layer, v.store, v.meta["rescale"], st))
        elif layer.kernel_size == (1, 1):
            assert layer.strides == (1, 1) and not layer.use_bias
            st = self._out_store(layer, out_t.shape)
            op = self._emit(PwOp(self, layer, "kernel", v, st))
            src = layer.inbound[0]
            # only for wide inputs (the 6x depthwise tensor in front of a project conv); the narrow block-input tensors in front of
            # expand convs take the fused dx+dW kernel instead
            op.fuse_input_bn = (v.bn is not None and v.store.c > layer.filters and v.store.parent is None
                                and len(self.cons.get(id(src), [])) == 1 and id(src) not in {id(t) for t in self.model.outputs})
        elif layer.kernel_size == (3, 3):
            assert layer.strides == (1, 1) and not layer.use_bias and layer.dilation_rate == (1, 1)
            st = self._out_store(layer, out_t.shape)
            op = self._emit(Conv3Op(self, layer, v, st))
            src = layer.inbound[0]
            # the narrow (<= 8 filters) form writes dx from a pointwise GEMM: the producer BN's backward sums can ride there
            op.fuse_input_bn = (v.bn is not None and layer.filters <= 8 and v.store.parent is None and v.store.ld == v.store.c
                                and len(self.cons.get(id(src), [])) == 1 and id(src) not in {id(t) for t in self.model.outputs})
        else:
            raise NotImplementedError(f"{layer.name}: Conv2D {layer.kernel_size} stride {layer.strides}")
        op.out_val = Val(st)
        st.producer = op
        setv(op.out_val)

    def _lower_concat(self, layer: K.Concatenate, ins: List[Val], setv):
        out_t = layer.outputs[0]
        if layer.axis_resolved == 1 and all("reshaped" in v.meta for v in ins):
            # SSD heads: (B, boxes_i, 4) blocks stacked along the anchor axis
            total = out_t.shape[1]
            st = Store(self, self.batch, total, 1, out_t.shape[2], layer.name)
            self.stores.append(st)
            off = 0
            for v in ins:
                self._emit(HeadGatherOp(self, Val(v.store, v.scale, v.shift, v.act, v.bn), st, off, total, f"{layer.name}:{v.store.name}"))
                off += v.meta["reshaped"][0]
            assert off == total
            setv(Val(st, head_concat=True))
            return
        assert layer.axis_resolved == 3, f"{layer.name}: unsupported concat axis"
        parent = self._concat_parts(layer)
        acts = set()
        off = 0
        copied_nonneg = True
        for t, v in zip(layer.inbound, ins):
            c = pad4(t.shape[-1])
            if v.store.parent is parent and v.store.coff == off:
                acts.add(v.meta.get("materialised_act", v.act))
            else:
                # not placed: copy the activated values into the slice (identity affine there)
                sl = parent.slice(off, c, f"{layer.name}[{off}:{off + c}]")
                self._emit(ApplyOp(self, v, None, sl, f"{layer.name}:copy{off}"))
                acts.add(None)
                copied_nonneg = copied_nonneg and _nonneg(v)
            off += c
        real = {a for a in acts if a is not None}
        if None in acts and real == {ACT_RELU} and copied_nonneg:
            # ShuffleNetV2 basic unit (models.py:573-598): the untouched half holds values >= 0 (it comes out of a ReLU'd
            # shuffle / max-pool), so the other half's lazy ReLU is the identity on it and the concat can stay a view
            setv(Val(parent, parent.wide_scale, parent.wide_shift, ACT_RELU))
        elif None in acts:
            # copied slices hold final values: only legal to keep lazy activations if there are none left
            assert not real or real == {ACT_NONE}, f"{layer.name}: cannot mix copied and lazily-activated inputs"
            setv(Val(parent))
        else:
            assert len(real) == 1, f"{layer.name}: concat inputs carry different activations {real}"
            setv(Val(parent, parent.wide_scale, parent.wide_shift, real.pop()))

    def _lower_softmax(self, layer: K.Softmax, v: Val, setv):
        out_t = layer.outputs[0]
        if "lazy_up" in v.meta:
            fy, fx = v.meta["lazy_up"]
            src: Val = v.meta["src"]
            n, h, w, c = (self.batch,) + tuple(out_t.shape[1:])
            prob = None
            if not self.training or self.keep_mask_probabilities:
                prob = Store(self, n, h, w, c, layer.name, need_grad=False)
                self.stores.append(prob)
            op = self._emit(MaskHeadOp(self, src, fy, fx, layer.name, prob))
            self.loss_ops[layer.name] = op
            setv(Val(prob if prob is not None else src.store, mask_head=op))
        elif v.meta.get("head_concat"):
            s = v.store
            st = Store(self, s.n, s.h, s.w, s.c, layer.name, need_grad=False)
            self.stores.append(st)
            self._emit(SoftmaxRowsOp(self, s, st, layer.name))
            setv(Val(st, logits=s))
        else:
            raise NotImplementedError(f"{layer.name}: Softmax on this tensor kind")

    def _lower_shufflenet(self, layer, ins, setv):
        """ShuffleNetV2-only layers (reference models.py:480-652): max-pool, channel split, channel shuffle"""
        out_t = layer.outputs[0]
        if isinstance(layer, K.MaxPooling2D):
            st = self._out_store(layer, out_t.shape)
            self._emit(MaxPoolOp(self, self._dense(ins[0], layer.name), st, layer.name))
            setv(Val(st, nonneg=_nonneg(ins[0])))
        elif isinstance(layer, L.Split):
            v = ins[0]
            assert v.scale is None and v.act == ACT_NONE and layer.axis in (-1, 3), f"{layer.name}: only plain channel splits are lowered"
            if any(t.shape[-1] % 4 != 0 for t in layer.outputs):
                # parts that are not whole 16-byte channel vectors: gather each into its own zero-padded tensor
                vd = self._dense(v, layer.name)
                outs = []
                for k, t in enumerate(layer.outputs):
                    st = Store(self, vd.store.n, vd.store.h, vd.store.w, pad4(t.shape[-1]), f"{layer.name}[{k}]")
                    self.stores.append(st)
                    outs.append(st)
                    self.vals[id(t)] = Val(st, nonneg=_nonneg(v))
                self._emit(SplitGatherOp(self, vd, outs, [int(t.shape[-1]) for t in layer.outputs], layer.name))
                return
            v.store.split_parent = True
            off = 0
            for t in layer.outputs:
                c = t.shape[-1]
                self.vals[id(t)] = Val(v.store.slice(off, c, f"{layer.name}[{off}:{off + c}]"), nonneg=_nonneg(v))   # zero-copy channel view
                off += c
        elif isinstance(layer, K.Permute):
            v = ins[0]
            assert v.meta.get("shuffle_groups") and layer.dims == (1, 2, 4, 3), f"{layer.name}: only the channel-shuffle Permute is lowered"
            setv(Val(v.store, shuffle_groups=v.meta["shuffle_groups"], shuffle_src=v.meta["shuffle_src"], shuffle_permuted=True))
        else:
            raise NotImplementedError(f"layer type {type(layer).__name__} ({layer.name}) is not lowered yet")

    def _lower_reshape(self, layer: K.Reshape, v: Val, setv):
        out_t = layer.outputs[0]
        tgt = tuple(out_t.shape[1:])
        if len(tgt) == 4:                          # (h, w, groups, c/groups): first half of a channel shuffle (models.py:497)
            setv(Val(v.store, v.scale, v.shift, v.act, v.bn, shuffle_groups=tgt[2], shuffle_src=v))
        elif v.meta.get("shuffle_permuted"):       # back to (h, w, c): emit the shuffle (models.py:503)
            st = self._out_store(layer, out_t.shape)
            src = v.meta["shuffle_src"]
            parts = getattr(src.store, "logical_parts", None)
            if parts is not None and any(cl % 4 != 0 for _, cl in parts):
                self._emit(TableShuffleOp(self, src, st, v.meta["shuffle_groups"], layer.name))
            else:
                self._emit(ShuffleOp(self, src, st, v.meta["shuffle_groups"], layer.name))
            setv(Val(st, nonneg=_nonneg(v.meta["shuffle_src"])))
        else:                                      # SSD heads: (B, H, W, boxes*4) -> (B, H*W*boxes, 4), metadata only
            setv(Val(v.store, v.scale, v.shift, v.act, v.bn, reshaped=tgt, **{k: x for k, x in v.meta.items() if k != "reshaped"}))

    keep_mask_probabilities = False

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

