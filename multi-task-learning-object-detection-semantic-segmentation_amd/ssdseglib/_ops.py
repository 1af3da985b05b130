"""What a `_graph.Model` is lowered to: tensor bookkeeping (`Store`, `BNRec`, `Val`) and one `Op` class per fused HIP launch family.
`_lowering.Lowering` builds the static launch list out of these and sets what an op or a store cannot know by itself (every such
attribute is declared here, with its default); `_engine.Engine` runs the list.  An op's `fwd` / `bwd` body is its part of that
list -- the calls into include/ssdseg.h, in order.
  * conv -> BatchNormalization(train) -> ReLU6 is never three passes: the conv kernel writes the RAW tensor once
    plus per-block (sum, sumsq); `bn_finalize` makes per-channel (scale, shift); every consumer applies
    act(scale*y+shift) while loading (`Val` below is that lazy view).  Backward mirrors it: one reduction pass per
    BN gives (k1, k0) and the producing conv's backward kernels form dY on load (gradient view).
  * Concatenate over channels is a write offset (producers write straight into their slice of the concat
    buffer, `ld` = total channels), Reshape/Split are metadata.
  * manual backward replaces autodiff: every op carries its own `bwd`; gradient fan-in order is the fixed reverse launch order.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _graph as K
from . import _hip as H
from . import layers as L

ACT_NONE, ACT_RELU, ACT_RELU6, ACT_ZERO = H.ACT_NONE, H.ACT_RELU, H.ACT_RELU6, H.ACT_ZERO


def _nonneg(v: "Val") -> bool:
    """values known to be >= 0 (a ReLU applied on top of them is the identity)"""
    return v.act in (ACT_RELU, ACT_RELU6, ACT_ZERO) or bool(v.meta.get("nonneg"))


def _act_of(relu: K.ReLU) -> int:
    if relu.max_value is None:
        return ACT_RELU
    if relu.max_value == 0.0:
        return ACT_ZERO          # quirk Q1: Keras clips to [0, 0]
    if relu.max_value == 6.0:
        return ACT_RELU6
    raise NotImplementedError(f"ReLU(max_value={relu.max_value}) is not used by ssdseglib")


class Store:
    """A tensor region resident in HBM: rows m = n*h*w, c channels, row stride ld (>= c for concat slices)."""

    def __init__(self, eng: "Engine", n, h, w, c, name, buf: Optional[H.DeviceBuffer] = None, ld: Optional[int] = None,
                 parent: Optional["Store"] = None, coff: int = 0, need_grad: bool = True):
        self.eng, self.n, self.h, self.w, self.c, self.name = eng, n, h, w, c, name
        self.m = n * h * w
        self.ld = c if ld is None else ld
        self.parent, self.coff = parent, coff
        self.buf = buf if buf is not None else eng.ctx.empty((self.m, self.ld))
        self.need_grad = need_grad
        self._grad: Optional[H.DeviceBuffer] = None
        self.gwritten = False
        self.pending = None        # (buffer, ld): deferred residual contribution to this gradient (see defer_residual)
        self.split_parent = False  # channel Split views write disjoint ranges of this gradient: zero it, then everyone accumulates
        self.stats: Optional[H.DeviceBuffer] = None   # per-block (sum, sumsq) partials from the producing conv
        self.nparts = 0
        # set by the lowering (`_lowering.Lowering`), None where it does not apply
        self.producer: Optional["Op"] = None   # the op that writes this store: BatchNormalization / ReLU re-point its `out_val`
        self.slice_scale = None    # a concat slice's range of its parent's wide_scale: the BatchNorm behind it writes its scale there
        self.slice_shift = None    # ... and its shift
        self.wide_scale = None     # a channel concat's per-channel scale over all its inputs (ones where an input has none)
        self.wide_shift = None     # ... and shift (zeros)
        self.logical_parts = None  # a channel concat's [(physical channel offset, logical width)] per input (TableShuffleOp)

    def slice(self, coff: int, c: int, name: str) -> "Store":
        assert coff + c <= self.c
        child = Store(self.eng, self.n, self.h, self.w, c, name, buf=self.buf.view(coff, (self.m * self.ld - coff,)), ld=self.ld,
                      parent=self, coff=coff, need_grad=self.need_grad)
        self.eng.stores.append(child)      # so its "gradient written" flag is reset with everyone else's each backward pass
        return child

    def _raw_grad(self) -> H.DeviceBuffer:
        if self._grad is None:
            if self.parent is not None:
                pg = self.parent._raw_grad()
                self._grad = pg.view(self.coff, (self.m * self.ld - self.coff,))
            else:
                self._grad = self.eng.ctx.zeros((self.m, self.ld))
        return self._grad

    @property
    def grad(self) -> H.DeviceBuffer:
        """the gradient buffer, complete as far as the backward pass has come (a deferred residual contribution is added first)"""
        self._materialise_pending()
        return self._raw_grad()

    def _written(self) -> bool:
        return self.gwritten or (self.parent is not None and self.parent.gwritten)

    def _materialise_pending(self):
        if self.pending is not None:
            buf, ld = self.pending
            self.pending = None
            self.eng.ctx.call("ssdseg_axpby", buf, ld, self._raw_grad(), self.ld, self.m, self.c, 1.0, 1.0 if self._written() else 0.0)
            self.gwritten = True

    def defer_residual(self, buf: H.DeviceBuffer, ld: int) -> bool:
        """Residual-Add backward: instead of copying the Add's output gradient into this (block input) gradient now, let the
        next writer -- the expand conv's backward-data GEMM -- add it in its epilogue.  False: not possible, copy as usual."""
        if self.parent is not None or self._written() or self.pending is not None or self.split_parent:
            return False
        self.pending = (buf, ld)
        return True

    def grad_slot(self) -> Tuple[H.DeviceBuffer, int]:
        """(gradient buffer, accumulate flag) for a consumer's backward; first writer overwrites."""
        self._materialise_pending()
        acc = 1 if self._written() else 0
        self.gwritten = True
        return self._raw_grad(), acc

    def grad_slot_residual(self):
        """as grad_slot for a writer whose kernel can add a residual tensor itself: (buffer, accumulate, residual, ldr)"""
        res, ldr = (None, 0)
        if self.pending is not None and not self._written():
            (res, ldr), self.pending = self.pending, None
        else:
            self._materialise_pending()
        acc = 1 if self._written() else 0
        self.gwritten = True
        return self._raw_grad(), acc, res, ldr


class BNRec:
    """Device state of one BatchNormalization layer."""

    def __init__(self, eng, layer: K.BatchNormalization, c: int, scale=None, shift=None):
        ctx = eng.ctx
        self.layer, self.c = layer, c
        self.gamma, self.beta = eng.param_view(layer, "gamma"), eng.param_view(layer, "beta")
        self.dgamma, self.dbeta = eng.grad_view(layer, "gamma"), eng.grad_view(layer, "beta")
        self.moving_mean, self.moving_var = eng.state_view(layer, "moving_mean"), eng.state_view(layer, "moving_variance")
        self.scale = scale if scale is not None else ctx.empty(c)
        self.shift = shift if shift is not None else ctx.empty(c)
        self.mean, self.invstd, self.k1, self.k0 = ctx.empty(c), ctx.empty(c), ctx.empty(c), ctx.empty(c)
        self.act = ACT_NONE
        self.bwd_done = False     # this step's backward reduction was already produced by a fused consumer kernel


class Val:
    """Lowered value of a symbolic tensor: a = act(scale * store + shift) (scale None -> act(store)).

    `meta` carries what one lowering rule leaves for a later one (`_lowering.Lowering`, by rule) or for `_loss_bind`; its keys:
      rescale            (scale, offset) of a Rescaling: set by _rescaling, read by _conv (the stem takes it)
      decode             the DecodeBoxesCentroidsOffsets layer: set by _decode, read by _nms
      suppress_with      the mask probabilities' store: set by _suppression, read by _nms
      lazy_up, src       an UpSampling2D that only a Softmax reads -- its size and its input Val: set by _upsampling, read by _softmax
      materialised_act   activation already applied to the stored values: set by _upsampling, read by _concat
      mask_head          the MaskHeadOp of the mask output: set by _softmax, read by _loss_bind
      logits             the pre-softmax store of the label output: set by _softmax, read by _loss_bind
      nms                the NonMaximumSuppression layer: set by _nms, read by _fit
      reshaped           target shape of an SSD head's Reshape: set by _reshape, read by _concat (the anchor-axis concat)
      head_concat        the (B, anchors, 4) concat of the heads: set by _concat, read by _softmax and _loss_bind
      shuffle_groups, shuffle_src, shuffle_permuted   the channel shuffle in progress (Reshape, Permute, Reshape): set by _reshape and
                         _permute, read by _permute and _reshape
      nonneg             stored values known to be >= 0: set by _maxpool, _split and _reshape, read by `_nonneg` (_concat)"""

    def __init__(self, store: Store, scale=None, shift=None, act=ACT_NONE, bn: Optional[BNRec] = None, **meta):
        self.store, self.scale, self.shift, self.act, self.bn = store, scale, shift, act, bn
        self.meta = meta

    def view(self) -> H.ViewStruct:
        return H.view(self.store.buf, self.scale, self.shift, self.act)

    def gview(self) -> H.GViewStruct:
        """gradient view of this value's RAW store for the backward of the op that produced the store"""
        s = self.store
        if self.bn is not None:
            b = self.bn
            return H.gview(s.grad, s.buf, b.scale, b.shift, b.k1, b.k0, b.act)
        return H.gview(s.grad)


# ====================================================================================================== ops
class Op:
    name = ""
    reach = frozenset()      # names of the model outputs that depend on this op (set when it is emitted: Lowering.emit, Engine._emit)

    def fwd(self):
        pass

    def bwd(self):
        pass


class StemOp(Op):
    def __init__(self, eng, layer: K.Conv2D, image: Store, rescale, out: Store):
        self.e, self.layer, self.image, self.rescale, self.out = eng, layer, image, rescale, out
        self.name = layer.name
        self.w = eng.param_view(layer, "kernel")
        self.b = eng.param_view(layer, "bias") if layer.use_bias else None
        self.dw = eng.grad_view(layer, "kernel")
        self.db = eng.grad_view(layer, "bias") if layer.use_bias else None
        if eng.training and self.b is None:
            # (a biased stem -- ShuffleNetV2, models.py:619 -- gets its batch statistics from a ChannelStatsOp instead: the fused
            # epilogue relies on padded rows being exactly zero)
            out.nparts = eng.ctx.parts("ssdseg_stem_conv_parts", image.n, image.h, image.w, out.c)
            out.stats = eng.ctx.empty((out.nparts, 2, out.c))
        self.out_val: Optional[Val] = None

    def fwd(self):
        i = self.image
        self.e.ctx.call("ssdseg_stem_conv_fwd", i.buf, self.w, self.b, self.out.buf, i.n, i.h, i.w, i.c, self.out.c,
                        self.rescale[0], self.rescale[1], self.out.stats if self.b is None else None)

    def bwd(self):
        i = self.image
        db = self.db
        if db is not None and self.out_val.bn is not None:
            # a bias in front of a training-mode BatchNormalization has an identically zero gradient (the batch mean absorbs
            # it); the reference's autodiff produces round-off noise there
            db.zero_()
            db = None
        self.e.ctx.call("ssdseg_stem_conv_bwd_weight", i.buf, self.out_val.gview(), self.dw, db, i.n, i.h, i.w, i.c, self.out.c,
                        self.rescale[0], self.rescale[1])


class DwOp(Op):
    def __init__(self, eng, layer, wname: str, inp: Val, out: Store, stride: int, dilation: int):
        self.e, self.layer, self.inp, self.out, self.stride, self.dilation = eng, layer, inp, out, stride, dilation
        self.name = layer.name + ":dw"
        self.w, self.dw = eng.param_view(layer, wname), eng.grad_view(layer, wname)
        s = inp.store
        if eng.training:
            out.nparts = eng.ctx.parts("ssdseg_dwconv_parts", s.n, s.h, s.w, s.c, stride, dilation)
            out.stats = eng.ctx.empty((out.nparts, 2, out.c))
        assert s.ld == s.c and out.ld == out.c, "depthwise kernels work on dense (non-sliced) tensors"
        self.out_val: Optional[Val] = None

    def fwd(self):
        s = self.inp.store
        self.e.ctx.call("ssdseg_dwconv_fwd", self.inp.view(), self.w, self.out.buf, s.n, s.h, s.w, s.c, self.stride, self.dilation,
                        self.out.stats)

    # set by the lowering when this conv is the only consumer of a BatchNorm(+ReLU) output, or the FIRST of several in layer
    # order -- i.e. the last one to contribute to that gradient in the backward pass (a backbone tap that also feeds the heads)
    fuse_input_bn = False

    def bwd(self):
        s = self.inp.store
        dx, acc = (s.grad_slot() if s.need_grad else (None, 0))
        b = self.inp.bn
        if self.fuse_input_bn and b is not None and dx is not None:
            # the kernel that completes dx also reduces the producer BN's (dgamma, dbeta, k1, k0): no second pass over the wide tensor
            self.e.ctx.call("ssdseg_dwconv_bwd_bn", self.inp.view(), self.w, self.out_val.gview(), dx, self.dw, s.n, s.h, s.w, s.c,
                            self.stride, self.dilation, acc, b.mean, b.invstd, b.dgamma, b.dbeta, b.k1, b.k0)
            b.bwd_done = True
            return
        self.e.ctx.call("ssdseg_dwconv_bwd", self.inp.view(), self.w, self.out_val.gview(), dx, self.dw, s.n, s.h, s.w, s.c, self.stride,
                        self.dilation, acc)


class PwOp(Op):
    def __init__(self, eng, layer, wname: str, inp: Val, out: Store):
        self.e, self.layer, self.inp, self.out = eng, layer, inp, out
        self.name = layer.name + ":pw"
        self.w, self.dw = eng.param_view(layer, wname), eng.grad_view(layer, wname)
        self.m, self.k, self.n = inp.store.m, inp.store.c, out.c
        if eng.training:
            out.nparts = eng.ctx.parts("ssdseg_pwconv_parts", self.m, self.n)
            out.stats = eng.ctx.empty((out.nparts, 2, self.n))
        self.out_val: Optional[Val] = None
        # the forward tile GEMM streams Wt[n][k]: one batched transposition per step for all layers (Engine._refresh_wt)
        self.wt = eng.register_wt(self.w, self.m, inp.store.ld, self.k, self.n)

    fuse_input_bn = False   # set by the lowering when this conv is the only consumer of a (wide) BatchNorm(+ReLU) output

    def fwd(self):
        self.e.ctx.call("ssdseg_pwconv_fwd_wt", self.inp.view(), self.inp.store.ld, self.w, self.wt, self.out.buf, self.out.ld, self.m, self.k,
                        self.n, self.out.stats)

    def bwd(self):
        s = self.inp.store
        gv = self.out_val.gview()
        b = self.inp.bn
        if (self.fuse_input_bn and b is not None and s.need_grad and s.pending is None and not s._written()):
            # sole consumer of a BatchNorm(+ReLU6) output (the depthwise BN in front of a project conv): that BN's backward
            # reduction rides in this conv's backward-data epilogue instead of a separate pass over (g, y)
            dx, _ = s.grad_slot()
            self.e.ctx.call("ssdseg_pwconv_bwd_bn", self.inp.view(), s.ld, gv, self.out.ld, self.w, dx, s.ld, self.dw, self.m, self.k, self.n,
                            b.mean, b.invstd, b.dgamma, b.dbeta, b.k1, b.k0)
            b.bwd_done = True
            return
        if s.need_grad:
            # dx and dW in one call: for few input channels (the expand convs) one kernel reads the wide gradient once
            dx, acc, res, ldr = s.grad_slot_residual()
            self.e.ctx.call("ssdseg_pwconv_bwd", self.inp.view(), s.ld, gv, self.out.ld, self.w, dx, s.ld, self.dw, self.m, self.k, self.n,
                            res, ldr, acc)
        else:
            self.e.ctx.call("ssdseg_pwconv_bwd_weight", self.inp.view(), s.ld, gv, self.out.ld, self.dw, self.m, self.k, self.n)


class Conv3Op(Op):
    def __init__(self, eng, layer, inp: Val, out: Store):
        self.e, self.layer, self.inp, self.out = eng, layer, inp, out
        self.name = layer.name + ":conv3x3"
        self.w, self.dw = eng.param_view(layer, "kernel"), eng.grad_view(layer, "kernel")
        s = inp.store
        if eng.training:
            out.nparts = eng.ctx.parts("ssdseg_conv3x3_parts", s.n, s.h, s.w, s.c, out.c)
            out.stats = eng.ctx.empty((out.nparts, 2, out.c))
        assert out.ld == out.c
        self.out_val: Optional[Val] = None
        # large layers (Winograd kernels): the forward leaves act(BN(x)) in a zero-bordered copy which the weight gradient reads
        # again, so the view is applied once per step (ssdseg_conv3x3_fwd_saved / _bwd_weight_saved)
        self.xsaved = None
        self.fuse_input_bn = False   # set by the lowering (narrow convs that are the only consumer of a BatchNorm output)
        if eng.training:
            need = C.c_longlong()
            H._check(eng.ctx.lib.ssdseg_conv3x3_saved_floats(s.n, s.h, s.w, s.c, out.c, C.byref(need)), "ssdseg_conv3x3_saved_floats")
            if need.value > 0:
                self.xsaved = eng.ctx.zeros(need.value)       # (the border stays zero for the life of the buffer)
        # the first channels of the input that an up-sampling op already writes into `xsaved` itself (set by the lowering together
        # with that op's `padded_out`, Lowering._upsampling_into_saved_input): the saved-input forward copies only the rest
        self.saved_from = 0

    def fwd(self):
        s = self.inp.store
        if self.xsaved is not None:
            c_from = self.saved_from if os.environ.get("SSDSEG_CONV3_PADFUSE", "1") != "0" else 0
            self.e.ctx.call("ssdseg_conv3x3_fwd_saved_from", self.inp.view(), s.ld, self.w, self.out.buf, s.n, s.h, s.w, s.c, self.out.c,
                            self.out.stats, self.xsaved, c_from)
            return
        self.e.ctx.call("ssdseg_conv3x3_fwd", self.inp.view(), s.ld, self.w, self.out.buf, s.n, s.h, s.w, s.c, self.out.c, self.out.stats)

    def bwd(self):
        s = self.inp.store
        gv = self.out_val.gview()
        if self.out_val.bn is not None:
            # both backward kernels read every dy element many times (9 taps): form dy = BN-backward(g, y) once, in place over g
            # (nothing else reads this g afterwards), and hand them the single-tensor identity view
            o = self.out
            self.e.ctx.call("ssdseg_gview_materialize", gv, o.ld, o.m, o.c)
            gv = H.gview(o.grad)
        # dW is off the critical path, but for a wide conv both backward kernels are bound by the SAME resource (the matrix pipes,
        # 0.8 of peak each on their own): side by side they only split the CUs and thrash each other's L2.  The side stream is
        # for pairing a weight gradient with an HBM-bound neighbour; here it is used only for the narrow (HBM-bound) 256 -> 4 conv.
        side = self.out.c <= 8 if os.environ.get("SSDSEG_CONV3_SIDE") is None else os.environ["SSDSEG_CONV3_SIDE"] == "1"
        if side:
            self.e.ctx.side(True)
        try:
            if self.xsaved is not None and self.out_val.bn is not None:     # (materialised dy: the saved-input weight gradient's form)
                self.e.ctx.call("ssdseg_conv3x3_bwd_weight_saved", self.xsaved, self.out.grad, self.dw, s.n, s.h, s.w, s.c, self.out.c)
            else:
                self.e.ctx.call("ssdseg_conv3x3_bwd_weight", self.inp.view(), s.ld, gv, self.dw, s.n, s.h, s.w, s.c, self.out.c)
        finally:
            if side:
                self.e.ctx.side(False)
        b = self.inp.bn
        if (self.fuse_input_bn and b is not None and s.need_grad and s.pending is None and not s._written()):
            # sole consumer of a BatchNorm(+ReLU) output (the decoder's logits conv behind sepconv-batchnorm): that BN's backward
            # sums ride in the epilogue of the GEMM that writes dx
            dx, _ = s.grad_slot()
            self.e.ctx.call("ssdseg_conv3x3_bwd_data_bn", self.inp.view(), gv, self.w, dx, s.ld, s.n, s.h, s.w, s.c, self.out.c,
                            b.mean, b.invstd, b.dgamma, b.dbeta, b.k1, b.k0)
            b.bwd_done = True
        elif s.need_grad:
            dx, acc = s.grad_slot()
            self.e.ctx.call("ssdseg_conv3x3_bwd_data", gv, self.w, dx, s.ld, s.n, s.h, s.w, s.c, self.out.c, acc)


class BnOp(Op):
    def __init__(self, eng, rec: BNRec, store: Store):
        self.e, self.rec, self.store = eng, rec, store
        self.name = rec.layer.name

    def fwd(self):
        r, s = self.rec, self.store
        l = r.layer
        if self.e.training:
            assert s.stats is not None, f"{self.name}: producer of {s.name} did not emit batch statistics"
            self.e.ctx.call("ssdseg_bn_finalize", s.stats, s.nparts, r.c, float(s.m), r.gamma, r.beta, l.epsilon, l.momentum, r.moving_mean,
                            r.moving_var, r.mean, r.invstd, r.scale, r.shift, 1)
        else:
            self.e.ctx.call("ssdseg_bn_finalize", None, 0, r.c, 0.0, r.gamma, r.beta, l.epsilon, l.momentum, r.moving_mean, r.moving_var,
                            None, None, r.scale, r.shift, 0)

    def bwd(self):
        r, s = self.rec, self.store
        if r.bwd_done:            # reduced by the consumer's backward kernel (DwOp.bwd)
            r.bwd_done = False
            return
        self.e.ctx.call("ssdseg_bn_bwd_reduce", s.grad, s.ld, s.buf, s.ld, s.m, r.c, r.scale, r.shift, r.mean, r.invstd, r.act, r.dgamma,
                        r.dbeta, r.k1, r.k0)


class ChannelStatsOp(Op):
    """batch statistics for a raw tensor whose producer has no fused stats epilogue"""

    def __init__(self, eng, store: Store):
        self.e, self.store = eng, store
        store.nparts = eng.ctx.parts("ssdseg_channel_stats_parts", store.m, store.c)
        store.stats = eng.ctx.empty((store.nparts, 2, store.c))

    def fwd(self):
        s = self.store
        self.e.ctx.call("ssdseg_channel_stats", s.buf, s.ld, s.m, s.c, s.stats)


class ApplyOp(Op):
    """out = view(a) (+ view(b)): Add, materialisation, copies into concat slices"""

    def __init__(self, eng, a: Val, b: Optional[Val], out: Store, name: str):
        self.e, self.a, self.b, self.out, self.name = eng, a, b, out, name

    def fwd(self):
        a, b, o = self.a, self.b, self.out
        self.e.ctx.call("ssdseg_bn_apply", a.view(), a.store.ld, b.view() if b is not None else None, b.store.ld if b is not None else 0,
                        o.buf, o.ld, o.m, o.c)

    # set by the lowering for an Add whose `a` (a projection's BN output) is consumed only here: it shares this op's output-gradient buffer
    alias_a = False

    def bwd(self):
        o = self.out
        og = o.grad
        for v in (self.a, self.b):
            if v is None or not v.store.need_grad:
                continue
            # d(out)/d(activated value) = 1 (the activation mask is applied by the producer's BN/ReLU backward)
            if v is self.a and self.alias_a:
                v.store.gwritten = True            # dL/da IS dL/dout: same buffer, no copy
                continue
            if v is self.b and self.b is not None and v.store.defer_residual(og, o.ld):
                continue                           # added by the next writer's GEMM epilogue (or on first read)
            g, acc = v.store.grad_slot()
            self.e.ctx.call("ssdseg_axpby", og, o.ld, g, v.store.ld, o.m, o.c, 1.0, 1.0 if acc else 0.0)


class ActBwdOp(Op):
    """backward-only: g *= act'(x) in place for an activation that sits on a materialised tensor"""

    def __init__(self, eng, store: Store, act: int, name):
        self.e, self.store, self.act, self.name = eng, store, act, name

    def bwd(self):
        s = self.store
        self.e.ctx.call("ssdseg_act_bwd", s.grad, s.ld, s.buf, s.ld, s.m, s.c, self.act)


class MaxPoolOp(Op):
    """MaxPooling2D(3, strides=2, 'same') (reference models.py:629)"""

    def __init__(self, eng, inp: Val, out: Store, name):
        self.e, self.inp, self.out, self.name = eng, inp, out, name

    def fwd(self):
        s = self.inp.store
        self.e.ctx.call("ssdseg_maxpool3x3s2_fwd", self.inp.view(), self.out.buf, s.n, s.h, s.w, s.c)

    def bwd(self):
        s = self.inp.store
        if s.need_grad:
            dx, acc = s.grad_slot()
            assert acc == 0, "max-pool input with another consumer"
            self.e.ctx.call("ssdseg_maxpool3x3s2_bwd", self.inp.view(), self.out.grad, dx, s.n, s.h, s.w, s.c)


class ShuffleOp(Op):
    """channel shuffle: Reshape(h, w, g, c/g) -> Permute(1, 2, 4, 3) -> Reshape(h, w, c) (reference models.py:497-503)"""

    def __init__(self, eng, inp: Val, out: Store, groups: int, name):
        self.e, self.inp, self.out, self.groups, self.name = eng, inp, out, groups, name

    def fwd(self):
        i, o = self.inp.store, self.out
        self.e.ctx.call("ssdseg_channel_shuffle", self.inp.view(), i.ld, o.buf, o.ld, i.m, i.c, self.groups, 0)

    def bwd(self):
        i, o = self.inp.store, self.out
        g, acc = i.grad_slot()     # gradient w.r.t. the ACTIVATED concat values; the branches' BN backward applies the masks
        assert acc == 0
        self.e.ctx.call("ssdseg_channel_shuffle", H.view(o.grad), o.ld, g, i.ld, i.m, i.c, self.groups, 1)


def pad4(c: int) -> int:
    """physical channel count of a tensor with c logical channels: the kernels work on 16-byte channel vectors, so a branch
    of 58 (ShuffleNetV2 '1x') or 122 ('2x') channels lives in a zero-padded 60- / 124-channel tensor"""
    return (int(c) + 3) // 4 * 4


class SplitGatherOp(Op):
    """channel Split whose parts are not multiples of 4 channels wide (ShuffleNetV2 '1x' / '2x', reference models.py:573):
    each part is gathered into its own zero-padded dense tensor; backward gathers the parts' gradients back"""

    def __init__(self, eng, inp: Val, outs: List[Store], widths: List[int], name):
        self.e, self.inp, self.outs, self.name = eng, inp, outs, name
        cin = inp.store.c
        self.tf, self.tb = [], []
        off = 0
        for st, w in zip(outs, widths):
            self.tf.append(eng.ctx.array(np.array([off + i if i < w else -1 for i in range(st.c)], np.int32)))
            self.tb.append(eng.ctx.array(np.array([j - off if off <= j < off + w else -1 for j in range(cin)], np.int32)))
            off += w

    def fwd(self):
        i = self.inp.store
        for st, t in zip(self.outs, self.tf):
            self.e.ctx.call("ssdseg_channel_gather", self.inp.view(), i.ld, st.buf, st.ld, i.m, st.c, t, 0)

    def bwd(self):
        i = self.inp.store
        g, acc = i.grad_slot()
        for k, (st, t) in enumerate(zip(self.outs, self.tb)):
            self.e.ctx.call("ssdseg_channel_gather", H.view(st.grad), st.ld, g, i.ld, i.m, i.c, t, 1 if (acc or k > 0) else 0)


class TableShuffleOp(Op):
    """channel shuffle of a concat whose parts carry padding channels: the permutation (reference models.py:497-503) composed
    with padded -> packed re-indexing, as one table lookup (the lazily fused BN + ReLU of the branches rides along, as in
    ShuffleOp); backward scatters through the inverse table (padding channels get zero gradient)"""

    def __init__(self, eng, inp: Val, out: Store, groups: int, name):
        self.e, self.inp, self.out, self.name = eng, inp, out, name
        parts = inp.store.logical_parts
        phys_of = [off + i for off, cl in parts for i in range(cl)]
        c_log = len(phys_of)
        assert c_log % groups == 0 and pad4(c_log) == out.c
        fwd = [phys_of[(j % groups) * (c_log // groups) + j // groups] if j < c_log else -1 for j in range(out.c)]
        inv = [-1] * inp.store.c
        for j, p in enumerate(fwd):
            if p >= 0:
                inv[p] = j
        self.tf, self.tb = eng.ctx.array(np.array(fwd, np.int32)), eng.ctx.array(np.array(inv, np.int32))

    def fwd(self):
        i, o = self.inp.store, self.out
        self.e.ctx.call("ssdseg_channel_gather", self.inp.view(), i.ld, o.buf, o.ld, i.m, o.c, self.tf, 0)

    def bwd(self):
        i, o = self.inp.store, self.out
        g, acc = i.grad_slot()
        assert acc == 0
        self.e.ctx.call("ssdseg_channel_gather", H.view(o.grad), o.ld, g, i.ld, i.m, i.c, self.tb, 0)


class GapOp(Op):
    def __init__(self, eng, inp: Val, out: Store, name):
        self.e, self.inp, self.out, self.name = eng, inp, out, name
        assert inp.store.ld == inp.store.c

    def fwd(self):
        s = self.inp.store
        self.e.ctx.call("ssdseg_gap_fwd", self.inp.view(), self.out.buf, s.n, s.h * s.w, s.c)

    def bwd(self):
        s = self.inp.store
        if s.need_grad:
            dx, acc = s.grad_slot()
            self.e.ctx.call("ssdseg_gap_bwd", self.out.grad, dx, s.n, s.h * s.w, s.c, acc)


class BilinearOp(Op):
    def __init__(self, eng, inp: Val, out: Store, fy: int, fx: int, name):
        self.e, self.inp, self.out, self.fy, self.fx, self.name = eng, inp, out, fy, fx, name

    # set by a Conv3Op that keeps a zero-bordered copy of its (concatenated) input: (buffer, row stride in floats) -- this op's
    # output then goes straight into the interior of that copy and the plain concat slice is not written (set by the lowering)
    padded_out = None

    def fwd(self):
        s = self.inp.store
        if self.padded_out is not None and os.environ.get("SSDSEG_CONV3_PADFUSE", "1") != "0":
            buf, ld = self.padded_out
            self.e.ctx.call("ssdseg_bilinear_fwd_padded", self.inp.view(), s.ld, buf, ld, s.n, s.h, s.w, s.c, self.fy, self.fx)
            return
        self.e.ctx.call("ssdseg_bilinear_fwd", self.inp.view(), s.ld, self.out.buf, self.out.ld, s.n, s.h, s.w, s.c, self.fy, self.fx)

    def bwd(self):
        s = self.inp.store
        if s.need_grad:
            dx, acc = s.grad_slot()
            self.e.ctx.call("ssdseg_bilinear_bwd", self.out.grad, self.out.ld, dx, s.ld, s.n, s.h, s.w, s.c, self.fy, self.fx, acc)


class MaskHeadOp(Op):
    """logits --bilinear x(fy,fx)--> softmax (= output-mask) [--> the bound mask loss, a `_loss_bind` variant]"""

    def __init__(self, eng, logits: Val, fy, fx, name, prob: Optional[Store]):
        self.e, self.logits, self.fy, self.fx, self.name, self.prob = eng, logits, fy, fx, name, prob
        s = logits.store
        assert logits.scale is None and logits.act == ACT_NONE and s.ld == s.c
        self.unbind()

    def unbind(self):
        """no loss bound: `_loss_bind.bind_losses` sets the variant and what every variant shares"""
        self.loss_impl = None
        self.y_true: Optional[H.DeviceBuffer] = None
        self.class_weights = None
        self.loss: Optional[H.DeviceBuffer] = None
        self.loss_scale = 0.0

    def fwd(self):
        s = self.logits.store
        prob = self.prob.buf if self.prob is not None else None
        if self.loss_impl is None:
            self.e.ctx.call("ssdseg_mask_head_fwd", s.buf, s.n, s.h, s.w, s.c, self.fy, self.fx, None, None, prob, None)
        else:
            self.loss_impl.fwd(self, prob)

    def bwd(self):
        if self.loss_impl is None:
            return
        g, acc = self.logits.store.grad_slot()
        assert acc == 0
        self.loss_impl.bwd(self, g)

    # read-only views of the bound variant's state (0 / None where it has none), for callers that ask the op
    kind = property(lambda self: self.loss_impl.kind)
    keep = property(lambda self: getattr(self.loss_impl, "keep", 0))
    pixel_loss = property(lambda self: getattr(self.loss_impl, "pixel_loss", None))
    thresh = property(lambda self: getattr(self.loss_impl, "thresh", None))
    kept = property(lambda self: getattr(self.loss_impl, "kept", None))


class HeadGatherOp(Op):
    """act(bn(head)) of one SSD feature map, viewed as (B, H*W*boxes, 4), written at its anchor offset of the
    (B, anchors, 4) concat (reference blocks.py:155 Reshape + models.py:256/271 Concatenate axis=1)"""

    def __init__(self, eng, inp: Val, out: Store, anchor_offset: int, anchors_total: int, name):
        self.e, self.inp, self.out, self.off, self.total, self.name = eng, inp, out, anchor_offset, anchors_total, name

    def fwd(self):
        s = self.inp.store
        self.e.ctx.call("ssdseg_head_gather", self.inp.view(), self.out.buf, s.n, s.h * s.w * s.c, s.c, self.off * 4, self.total * 4, 0)

    def bwd(self):
        s = self.inp.store
        g, acc = s.grad_slot()
        assert acc == 0
        self.e.ctx.call("ssdseg_head_gather", H.view(self.out.grad), g, s.n, s.h * s.w * s.c, s.c, self.off * 4, self.total * 4, 1)


class SoftmaxRowsOp(Op):
    def __init__(self, eng, inp: Store, out: Store, name):
        self.e, self.inp, self.out, self.name = eng, inp, out, name

    def fwd(self):
        self.e.ctx.call("ssdseg_softmax_rows", H.view(self.inp.buf), self.out.buf, self.inp.m, self.inp.c)


class DetLossOp(Op):
    """confidence + localization losses, one `_loss_bind` variant each (`conf_impl`: mined or focal; `loc_impl`: smooth-L1, fused into
    the confidence entry, or the IoU family, an entry of its own called after it on the same stream).  The gradients w.r.t. the
    pre-softmax logits / box offsets are produced in the forward call (fused), each scaled by its own loss weight / batch, and simply
    stay in the concat stores' gradient buffers."""

    def __init__(self, eng, logits: Store, probs: Store, boxes: Store):
        self.e, self.logits, self.probs, self.boxes = eng, logits, probs, boxes
        self.name = "det-loss"
        b, a = probs.n, probs.h * probs.w
        self.y_labels, self.y_boxes = eng.ctx.empty((b, a, probs.c)), eng.ctx.empty((b, a, 4))
        self.conf_loss, self.loc_loss = eng.ctx.empty(b), eng.ctx.empty(b)
        self.conf_impl = self.loc_impl = None   # the two variants and their weights: `_loss_bind.bind_losses`, afresh on every call
        self.w_conf = self.w_loc = 1.0

    def fwd(self):
        p = self.probs
        tr = self.e.training
        fused = self.loc_impl.fused                # else the confidence entry runs without its smooth-L1 half: both loc outputs NULL
        ins = (self.y_labels, p.buf, self.y_boxes, self.boxes.buf, p.n, p.h * p.w, p.c)
        outs = (self.conf_loss, self.loc_loss if fused else None, self.logits.grad if tr else None,
                self.boxes.grad if tr and fused else None)
        self.conf_impl.fwd(self, ins, outs)
        self.loc_impl.fwd(self)

    def bwd(self):
        self.logits.gwritten = True
        self.boxes.gwritten = True

    # read-only views of the bound variants: "mined" | "focal"; the losses.iou_localization_loss callable (None: smooth-L1) and its number
    kind = property(lambda self: self.conf_impl.kind)
    loc = property(lambda self: self.loc_impl.fn)
    loc_kind = property(lambda self: self.loc_impl.kind)


class DecodeNmsOp(Op):
    def __init__(self, eng, boxes: Store, probs: Store, decode: L.DecodeBoxesCentroidsOffsets, nms: L.NonMaximumSuppression,
                 suppress_with: Optional[Store], out: Store):
        self.e, self.boxes, self.probs, self.nms, self.mask, self.out = eng, boxes, probs, nms, suppress_with, out
        ctx = eng.ctx
        a = boxes.h * boxes.w
        cent = np.stack([decode.center_x_boxes_default, decode.center_y_boxes_default, decode.width_boxes_default,
                         decode.height_boxes_default], axis=1).astype(np.float32)
        assert cent.shape == (a, 4)
        self.centroids = ctx.array(cent)
        self.stds = (C.c_float * 4)(decode.standard_deviation_center_x_offsets, decode.standard_deviation_center_y_offsets,
                                    decode.standard_deviation_width_offsets, decode.standard_deviation_height_offsets)
        self.corners = ctx.empty((boxes.n, a, 4))
        self.probs_s = ctx.empty((probs.n, a, probs.c)) if suppress_with is not None else None
        self.valid = ctx.empty(boxes.n, np.int32)
        self.name = nms.name
        self.defer_nms = False      # fwd() stops after decode + suppression; the caller runs run_nms() itself (run_evaluate)

    def decode(self):
        """decoded corners and the (segmentation-suppressed) probabilities: everything of the tail that does not depend on the
        two NMS thresholds"""
        b, a = self.boxes.n, self.boxes.h * self.boxes.w
        ctx = self.e.ctx
        ctx.call("ssdseg_decode_boxes", self.boxes.buf, self.centroids, b, a, self.stds, self.corners)
        if self.mask is not None:
            m = self.mask
            ctx.call("ssdseg_seg_suppress", m.buf, m.m, m.c, self.probs.buf, b * a, self.probs_s)

    def run_nms(self, boxes_iou_threshold=None, labels_probability_threshold=None, soft_nms_sigma=None, out: Optional[H.DeviceBuffer] = None):
        """the NMS call alone on what decode() left, with the layer's thresholds and Soft-NMS sigma or the given ones (a threshold
        grid re-runs only this: NB03#cell21), into the op's output or `out` [b][max_total][6].  A sigma of 0 is the hard NMS,
        ssdseg_combined_nms as ever; above 0 ssdseg_combined_nms_soft"""
        b, a, c = self.boxes.n, self.boxes.h * self.boxes.w, self.probs.c
        n = self.nms
        iou = n.boxes_iou_threshold if boxes_iou_threshold is None else boxes_iou_threshold
        prob = n.labels_probability_threshold if labels_probability_threshold is None else labels_probability_threshold
        sigma = n.soft_nms_sigma if soft_nms_sigma is None else L.soft_nms_sigma_value(soft_nms_sigma)
        probs = self.probs_s if self.mask is not None else self.probs.buf
        limits = (n.max_number_of_boxes_per_class, n.max_number_of_boxes_per_sample, float(iou), float(prob))
        dst = self.out.buf if out is None else out
        if sigma == 0:
            self.e.ctx.call("ssdseg_combined_nms", self.corners, probs, b, a, c, *limits, dst, self.valid)
        else:
            self.e.ctx.call("ssdseg_combined_nms_soft", self.corners, probs, b, a, c, *limits, float(sigma), dst, self.valid)

    def fwd(self):
        self.decode()
        if not self.defer_nms:
            self.run_nms()


