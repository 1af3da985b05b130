"""The lowering: a `_graph.Model` -> the engine's static list of `_ops` launches, its stores and the `Val` of every symbolic tensor.
One `Lowering` lives for one `Engine` construction: it owns what only construction needs (the consumer map, the model-output set,
the concat placement plan, the concat buffers, the reach of the layer at hand) and leaves its results on the engine under the names
the other modules read (`ops`, `stores`, `vals`, `loss_ops`, `input_store`).  Ops and stores take the engine (for `ctx`, the
parameter views and `stores`), never the builder, and this module never imports `_engine`.

A fusion decision is written once: `sole_consumer` and `first_consumer` are the two questions about who else reads a tensor,
`_produced` / `_wrapped` tie a producing op to its store and to the `Val` its backward reads.  A new layer kind is one method and
one row of `Lowering.RULES`.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from . import _graph as K
from . import layers as L
from ._ops import (ACT_NONE, ACT_RELU, ActBwdOp, ApplyOp, BilinearOp, BNRec, BnOp, ChannelStatsOp, Conv3Op, DecodeNmsOp, DwOp, GapOp,
                   HeadGatherOp, MaskHeadOp, MaxPoolOp, Op, PwOp, ShuffleOp, SoftmaxRowsOp, SplitGatherOp, StemOp, Store, TableShuffleOp,
                   Val, _act_of, _nonneg, pad4)


# ====================================================================================================== who reads a tensor
def consumers(model: K.Model) -> Dict[int, List[K.Layer]]:
    """id(tensor) -> the layers that read it, in layer order"""
    cons: Dict[int, List[K.Layer]] = {}
    for l in model.layers:
        for t in l.inbound:
            cons.setdefault(id(t), []).append(l)
    return cons


def sole_consumer(cons, out_ids, t) -> bool:
    """`t` has exactly one consumer and is not a model output: whatever that consumer does to `t` or to its gradient (write it
    in place, fold the producer BatchNorm's backward sums into its own kernel, share a gradient buffer) nobody else can see"""
    return len(cons.get(id(t), ())) == 1 and id(t) not in out_ids


def first_consumer(cons, t, layer) -> bool:
    """`layer` is the first consumer of `t` in layer order.  NOT `sole_consumer` on purpose: the first reader in layer order is the
    LAST contributor to dL/dt in the backward pass, so its kernel sees the completed gradient and may take the producer
    BatchNorm's backward sums over it even though others read `t` too (and even if `t` is a model output) -- the block-13 tap
    feeds the ASPP and the first SSD head behind block 13's depthwise conv, which completes its gradient"""
    readers = cons.get(id(t), ())
    return bool(readers) and readers[0] is layer


def plan_concats(model: K.Model, cons, out_ids) -> Dict[int, Tuple[K.Concatenate, int]]:
    """channel-axis Concatenate: let each input's storage producer write straight into its slice
    -> id(producer layer) -> (concat layer, channel offset)"""
    placement: Dict[int, Tuple[K.Concatenate, int]] = {}
    for l in model.layers:
        if not isinstance(l, K.Concatenate) or l.axis_resolved != 3:
            continue
        off = 0
        for t in l.inbound:
            c = pad4(t.shape[-1])
            cur, ok = t, True
            # walk back through lazily-fused per-channel layers to whoever writes memory
            while isinstance(cur.layer, (K.ReLU, K.BatchNormalization)):
                if not sole_consumer(cons, out_ids, cur):
                    ok = False
                    break
                cur = cur.layer.inbound[0]
            prod = cur.layer
            if ok and isinstance(prod, (K.Conv2D, K.SeparableConv2D, K.UpSampling2D)) and sole_consumer(cons, out_ids, cur) \
                    and not (isinstance(prod, K.Conv2D) and prod.kernel_size == (3, 3)):
                placement[id(prod)] = (l, off)
            off += c
    return placement


def outputs_reached(model: K.Model, cons) -> Dict[int, frozenset]:
    """id(layer) -> names of the model outputs that depend on it"""
    names = {id(t): t.layer.name for t in model.outputs}
    reach: Dict[int, frozenset] = {}
    for layer in reversed(model.layers):
        r = set()
        for t in layer.outputs:
            if id(t) in names:
                r.add(names[id(t)])
            for c in cons.get(id(t), []):
                r |= reach.get(id(c), frozenset())
        reach[id(layer)] = frozenset(r)
    return reach


# ====================================================================================================== the builder
class Lowering:
    def __init__(self, eng):
        self.e, self.model, self.batch, self.training, self.ctx = eng, eng.model, eng.batch, eng.training, eng.ctx
        self.cons = consumers(self.model)
        self.out_ids = {id(t) for t in self.model.outputs}
        self.placement = plan_concats(self.model, self.cons, self.out_ids)
        self.concat_store: Dict[int, Store] = {}
        self.reach = frozenset()            # of the layer being lowered: every op it emits carries it (_branches.plan_branches)
        self.vals = eng.vals

    def run(self):
        reach = outputs_reached(self.model, self.cons)
        for layer in self.model.layers:
            self.reach = reach[id(layer)]
            for cls in type(layer).__mro__:
                if cls in self.RULES:
                    break
            else:
                raise NotImplementedError(f"layer type {type(layer).__name__} ({layer.name}) is not lowered yet")
            ins = [self.vals[id(t)] for t in layer.inbound]
            v = self.RULES[cls](self, layer, ins)
            if v is not None:                       # (Split sets one Val per output itself)
                self.vals[id(layer.outputs[0])] = v

    # ------------------------------------------------------------------ helpers
    def sole(self, t) -> bool:
        return sole_consumer(self.cons, self.out_ids, t)

    def emit(self, op: Op):
        op.reach = self.reach
        self.e.ops.append(op)
        return op

    def store(self, n, h, w, c, name, **kw) -> Store:
        st = Store(self.e, n, h, w, c, name, **kw)
        self.e.stores.append(st)
        return st

    @staticmethod
    def _produced(op: Op, st: Store) -> Val:
        """`op` writes `st`: the store knows its producer, and the producer's backward reads dL/d(st) through `out_val` -- the raw
        store until a BatchNormalization (+ReLU) wraps it (`_wrapped`)"""
        st.producer = op
        op.out_val = Val(st)
        return op.out_val

    @staticmethod
    def _wrapped(st: Store, nv: Val) -> Val:
        """BatchNormalization / ReLU made `nv` out of the raw `st`: its producer's backward forms dY through that view from now on"""
        if st.producer is not None:
            st.producer.out_val = nv
        return nv

    def _concat_parts(self, concat: K.Concatenate) -> Store:
        """the store of a channel concat (with its wide scale and shift), created on first use"""
        key = id(concat)
        if key not in self.concat_store:
            n, h, w, _ = (self.batch,) + tuple(concat.outputs[0].shape[1:])
            parts, c = [], 0                       # physical layout: every input at its padded width
            for t in concat.inbound:
                parts.append((c, int(t.shape[-1])))
                c += pad4(t.shape[-1])
            st = Store(self.e, n, h, w, c, concat.name)
            st.logical_parts = parts
            st.wide_scale = self.ctx.array(np.ones(c, np.float32))
            st.wide_shift = self.ctx.array(np.zeros(c, np.float32))
            self.concat_store[key] = st
            self.e.stores.append(st)
        return self.concat_store[key]

    def _out_store(self, layer, shape, name=None) -> Store:
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
        return self.store(n, h, w, c, name or layer.name)

    def _dense(self, v: Val, name: str) -> Val:
        """a Val over a dense store (materialise sliced / strided inputs for kernels that need ld == c)"""
        if v.store.ld == v.store.c:
            return v
        s = v.store
        st = self.store(s.n, s.h, s.w, s.c, name + ":dense")
        self.emit(ApplyOp(self.e, v, None, st, name + ":dense"))
        return Val(st)

    # ------------------------------------------------------------------ one rule per layer kind: (layer, input Vals) -> output Val
    def _input(self, layer, ins):
        n, h, w, c = (self.batch,) + tuple(layer.outputs[0].shape[1:])
        self.e.input_store = self.store(n, h, w, c, layer.name, need_grad=False)
        return Val(self.e.input_store)

    def _rescaling(self, layer, ins):
        return Val(ins[0].store, rescale=(layer.scale, layer.offset))

    def _conv(self, layer: K.Conv2D, ins):
        v, src, out_t = ins[0], layer.inbound[0], layer.outputs[0]
        if "rescale" in v.meta:
            assert layer.kernel_size == (3, 3) and layer.strides == (2, 2), "Rescaling must feed the 3x3 stride-2 stem"
            st = self._out_store(layer, out_t.shape)
            op = self.emit(StemOp(self.e, layer, v.store, v.meta["rescale"], st))
        elif layer.kernel_size == (1, 1):
            assert layer.strides == (1, 1) and not layer.use_bias
            st = self._out_store(layer, out_t.shape)
            op = self.emit(PwOp(self.e, layer, "kernel", v, st))
            # only for wide inputs (the 6x depthwise tensor in front of a project conv); the narrow block-input tensors in front of
            # expand convs take the fused dx+dW kernel instead
            op.fuse_input_bn = v.bn is not None and v.store.c > layer.filters and v.store.parent is None and self.sole(src)
        elif layer.kernel_size == (3, 3):
            assert layer.strides == (1, 1) and not layer.use_bias and layer.dilation_rate == (1, 1)
            st = self._out_store(layer, out_t.shape)
            op = Conv3Op(self.e, layer, v, st)
            self._upsampling_into_saved_input(op, src)
            self.emit(op)
            # the narrow (<= 8 filters) form writes dx from a pointwise GEMM: the producer BN's backward sums can ride there
            op.fuse_input_bn = (v.bn is not None and layer.filters <= 8 and v.store.parent is None and v.store.ld == v.store.c
                                and self.sole(src))
        else:
            raise NotImplementedError(f"{layer.name}: Conv2D {layer.kernel_size} stride {layer.strides}")
        return self._produced(op, st)

    def _upsampling_into_saved_input(self, op: Conv3Op, src):
        """The input of the DeepLabV3+ decoder conv is Concatenate(up-sampled ASPP output, backbone branch) (blocks.py:104-113).  The
        up-sampling writes final (already activated) values into channels [0, c) of the concat buffer, which the saved-input
        forward then copies into the zero-bordered buffer.  Nothing else reads those channels of the plain concat buffer, so the
        up-sampling writes them into the bordered buffer directly and the copy shrinks to the other branch's channels."""
        s = op.inp.store
        if op.xsaved is None or s.ld != s.c:
            return
        ops = self.e.ops
        up = [o for o in ops if isinstance(o, BilinearOp) and o.out.parent is s and o.out.coff == 0 and o.out.ld == s.c
              and o.out.h == s.h and o.out.w == s.w]
        users = [o for o in ops if any((getattr(v, "store", v) is s) for v in vars(o).values())]
        if len(up) == 1 and not users and self.sole(src):
            up[0].padded_out = (op.xsaved, s.c)
            op.saved_from = up[0].out.c

    def _depthwise(self, layer: K.DepthwiseConv2D, ins):
        assert layer.strides[0] == layer.strides[1] and layer.dilation_rate[0] == layer.dilation_rate[1]
        st = self._out_store(layer, layer.outputs[0].shape)
        op = self.emit(DwOp(self.e, layer, "depthwise_kernel", self._dense(ins[0], layer.name), st, layer.strides[0], layer.dilation_rate[0]))
        op.fuse_input_bn = (op.inp is ins[0] and ins[0].bn is not None and ins[0].store.parent is None
                            and first_consumer(self.cons, layer.inbound[0], layer) and layer.dilation_rate[0] == 1)
        return self._produced(op, st)

    def _separable(self, layer: K.SeparableConv2D, ins):
        assert layer.strides[0] == layer.strides[1] and layer.dilation_rate[0] == layer.dilation_rate[1]
        inp = self._dense(ins[0], layer.name)
        n, h, w, _ = (self.batch,) + tuple(layer.outputs[0].shape[1:])
        mid = self.store(n, h, w, inp.store.c, layer.name + ":dw")
        dw = self.emit(DwOp(self.e, layer, "depthwise_kernel", inp, mid, layer.strides[0], layer.dilation_rate[0]))
        # sole consumer of a BatchNorm(+ReLU) output (the decoder's sepconv behind the 3x3 conv): that BN's backward sums
        # ride in the depthwise backward, as for the MBConv blocks
        dw.fuse_input_bn = inp is ins[0] and ins[0].bn is not None and ins[0].store.parent is None and self.sole(layer.inbound[0])
        mid.stats = None   # no BatchNormalization between the two halves
        st = self._out_store(layer, layer.outputs[0].shape)
        pw = self.emit(PwOp(self.e, layer, "pointwise_kernel", self._produced(dw, mid), st))
        return self._produced(pw, st)

    def _batchnorm(self, layer: K.BatchNormalization, ins):
        v = ins[0]
        assert v.scale is None and v.act == ACT_NONE and v.bn is None, f"{layer.name}: BatchNormalization input must be a raw conv output"
        st = v.store
        rec = BNRec(self.e, layer, st.c, st.slice_scale, st.slice_shift)
        if self.training and st.stats is None:
            self.emit(ChannelStatsOp(self.e, st))
        self.emit(BnOp(self.e, rec, st))
        return self._wrapped(st, Val(st, rec.scale, rec.shift, ACT_NONE, rec))

    def _relu(self, layer: K.ReLU, ins):
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
                self.emit(ActBwdOp(self.e, v.store, act, layer.name))
        nv = Val(v.store, v.scale, v.shift, act, v.bn)
        return self._wrapped(v.store, nv) if v.bn is not None else nv

    def _add(self, layer: K.Add, ins):
        st = self._out_store(layer, layer.outputs[0].shape)
        op = self.emit(ApplyOp(self.e, ins[1], ins[0], st, layer.name))
        a = ins[1]
        if (self.training and a.bn is not None and a.store.parent is None and st.parent is None and a.store.ld == st.ld and a.store.c == st.c
                and self.sole(layer.inbound[1])):
            a.store._grad = st._raw_grad()    # dL/d(projection output) == dL/d(Add output): one buffer
            op.alias_a = True
        return Val(st)

    def _concat(self, layer: K.Concatenate, ins: List[Val]):
        out_t = layer.outputs[0]
        if layer.axis_resolved == 1 and all("reshaped" in v.meta for v in ins):
            # SSD heads: (B, boxes_i, 4) blocks stacked along the anchor axis
            total = out_t.shape[1]
            st = self.store(self.batch, total, 1, out_t.shape[2], layer.name)
            off = 0
            for v in ins:
                self.emit(HeadGatherOp(self.e, Val(v.store, v.scale, v.shift, v.act, v.bn), st, off, total, f"{layer.name}:{v.store.name}"))
                off += v.meta["reshaped"][0]
            assert off == total
            return Val(st, head_concat=True)
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
                self.emit(ApplyOp(self.e, v, None, sl, f"{layer.name}:copy{off}"))
                acts.add(None)
                copied_nonneg = copied_nonneg and _nonneg(v)
            off += c
        real = {a for a in acts if a is not None}
        if None in acts and real == {ACT_RELU} and copied_nonneg:
            # ShuffleNetV2 basic unit (models.py:573-598): the untouched half holds values >= 0 (it comes out of a ReLU'd
            # shuffle / max-pool), so the other half's lazy ReLU is the identity on it and the concat can stay a view
            return Val(parent, parent.wide_scale, parent.wide_shift, ACT_RELU)
        if None in acts:
            # copied slices hold final values: only legal to keep lazy activations if there are none left
            assert not real or real == {ACT_NONE}, f"{layer.name}: cannot mix copied and lazily-activated inputs"
            return Val(parent)
        assert len(real) == 1, f"{layer.name}: concat inputs carry different activations {real}"
        return Val(parent, parent.wide_scale, parent.wide_shift, real.pop())

    def _gap(self, layer, ins):
        st = self._out_store(layer, layer.outputs[0].shape)
        self.emit(GapOp(self.e, self._dense(ins[0], layer.name), st, layer.name))
        return Val(st)

    def _upsampling(self, layer: K.UpSampling2D, ins):
        out_t, v = layer.outputs[0], ins[0]
        cons = self.cons.get(id(out_t), [])
        if len(cons) == 1 and isinstance(cons[0], K.Softmax):
            return Val(v.store, v.scale, v.shift, v.act, v.bn, lazy_up=layer.size, src=v)
        st = self._out_store(layer, out_t.shape)
        self.emit(BilinearOp(self.e, v, st, layer.size[0], layer.size[1], layer.name))
        # values are already activated; the concat-wide activation is idempotent on them
        return Val(st, materialised_act=v.act)

    def _softmax(self, layer: K.Softmax, ins):
        v, out_t = ins[0], layer.outputs[0]
        if "lazy_up" in v.meta:
            fy, fx = v.meta["lazy_up"]
            src: Val = v.meta["src"]
            n, h, w, c = (self.batch,) + tuple(out_t.shape[1:])
            prob = None
            if not self.training or self.e.keep_mask_probabilities:
                prob = self.store(n, h, w, c, layer.name, need_grad=False)
            op = self.emit(MaskHeadOp(self.e, src, fy, fx, layer.name, prob))
            self.e.loss_ops[layer.name] = op
            return Val(prob if prob is not None else src.store, mask_head=op)
        if v.meta.get("head_concat"):
            s = v.store
            st = self.store(s.n, s.h, s.w, s.c, layer.name, need_grad=False)
            self.emit(SoftmaxRowsOp(self.e, s, st, layer.name))
            return Val(st, logits=s)
        raise NotImplementedError(f"{layer.name}: Softmax on this tensor kind")

    def _reshape(self, layer: K.Reshape, ins):
        v, out_t = ins[0], layer.outputs[0]
        tgt = tuple(out_t.shape[1:])
        if len(tgt) == 4:                          # (h, w, groups, c/groups): first half of a channel shuffle (models.py:497)
            return Val(v.store, v.scale, v.shift, v.act, v.bn, shuffle_groups=tgt[2], shuffle_src=v)
        if v.meta.get("shuffle_permuted"):         # back to (h, w, c): emit the shuffle (models.py:503)
            st = self._out_store(layer, out_t.shape)
            src = v.meta["shuffle_src"]
            parts = src.store.logical_parts
            if parts is not None and any(cl % 4 != 0 for _, cl in parts):
                self.emit(TableShuffleOp(self.e, src, st, v.meta["shuffle_groups"], layer.name))
            else:
                self.emit(ShuffleOp(self.e, src, st, v.meta["shuffle_groups"], layer.name))
            return Val(st, nonneg=_nonneg(v.meta["shuffle_src"]))
        # SSD heads: (B, H, W, boxes*4) -> (B, H*W*boxes, 4), metadata only
        return Val(v.store, v.scale, v.shift, v.act, v.bn, reshaped=tgt, **{k: x for k, x in v.meta.items() if k != "reshaped"})

    def _decode(self, layer, ins):
        return Val(ins[0].store, decode=layer)

    def _suppression(self, layer, ins):
        return Val(ins[1].store, suppress_with=ins[0].store)

    def _nms(self, layer: L.NonMaximumSuppression, ins):
        boxes_v, probs_v = ins[0], ins[1]
        out = self.store(self.batch, layer.max_number_of_boxes_per_sample, 1, 6, layer.name, need_grad=False)
        self.emit(DecodeNmsOp(self.e, boxes_v.store, probs_v.store, boxes_v.meta["decode"], layer, probs_v.meta.get("suppress_with"), out))
        return Val(out, nms=layer)

    # ShuffleNetV2-only layers (reference models.py:480-652): max-pool, channel split, channel shuffle
    def _maxpool(self, layer, ins):
        st = self._out_store(layer, layer.outputs[0].shape)
        self.emit(MaxPoolOp(self.e, self._dense(ins[0], layer.name), st, layer.name))
        return Val(st, nonneg=_nonneg(ins[0]))

    def _split(self, layer: L.Split, ins):
        v = ins[0]
        assert v.scale is None and v.act == ACT_NONE and layer.axis in (-1, 3), f"{layer.name}: only plain channel splits are lowered"
        if any(t.shape[-1] % 4 != 0 for t in layer.outputs):
            # parts that are not whole 16-byte channel vectors: gather each into its own zero-padded tensor
            vd = self._dense(v, layer.name)
            outs = []
            for k, t in enumerate(layer.outputs):
                st = self.store(vd.store.n, vd.store.h, vd.store.w, pad4(t.shape[-1]), f"{layer.name}[{k}]")
                outs.append(st)
                self.vals[id(t)] = Val(st, nonneg=_nonneg(v))
            self.emit(SplitGatherOp(self.e, vd, outs, [int(t.shape[-1]) for t in layer.outputs], layer.name))
            return None
        v.store.split_parent = True
        off = 0
        for t in layer.outputs:
            c = t.shape[-1]
            self.vals[id(t)] = Val(v.store.slice(off, c, f"{layer.name}[{off}:{off + c}]"), nonneg=_nonneg(v))   # zero-copy channel view
            off += c
        return None

    def _permute(self, layer: K.Permute, ins):
        v = ins[0]
        assert v.meta.get("shuffle_groups") and layer.dims == (1, 2, 4, 3), f"{layer.name}: only the channel-shuffle Permute is lowered"
        return Val(v.store, shuffle_groups=v.meta["shuffle_groups"], shuffle_src=v.meta["shuffle_src"], shuffle_permuted=True)

    # layer class -> rule, looked up along the layer's MRO (no class here derives from another: their order says nothing)
    RULES = {K.InputLayer: _input, K.Rescaling: _rescaling, K.Conv2D: _conv, K.DepthwiseConv2D: _depthwise, K.SeparableConv2D: _separable,
             K.BatchNormalization: _batchnorm, K.ReLU: _relu, K.Add: _add, K.Concatenate: _concat, K.GlobalAveragePooling2D: _gap,
             K.UpSampling2D: _upsampling, K.Softmax: _softmax, K.Reshape: _reshape, L.DecodeBoxesCentroidsOffsets: _decode,
             L.SegmentationSuppression: _suppression, L.NonMaximumSuppression: _nms, K.MaxPooling2D: _maxpool, L.Split: _split,
             K.Permute: _permute}
