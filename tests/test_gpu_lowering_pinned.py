"""GPU: what building an engine allocates and lowers to, how it schedules its branches and what one pass hands to the C library --
pinned, argument for argument.

The lowering of a `_graph.Model` (ssdseglib/_lowering.py) and the branch schedule (`plan_branches`) were carved out of `Engine`.
Nothing a step launches may move with that: not the op list, not a store, not the order of the device allocations made while an
engine is built and bound (a changed order moves every later buffer, which is a change under every benchmark), not one argument of
one C call.  Each case below builds an engine the way the parity tests build theirs and writes ONE text from an explicit list of
fields (never `vars()`: an attribute declared later cannot change it):

  1. every owned device allocation made during construction and binding, in order: (ordinal, bytes, dtype);
  2. every op in order: class, name, sorted reach, fuse_input_bn, alias_a, and every Store it holds directly or through a Val:
     name, (n, h, w, c), ld, coff, parent name, need_grad, nparts (a Val adds its activation and its BatchNorm's layer and act);
  3. for training engines, the four lists of `_schedule()` by op name;
  4. the trace of every `Context.call` of one `train_step` (training engines) or one `forward()` (the others) on inputs built from
     integer arithmetic: the entry name, every scalar, host arrays by value, and every device pointer -- the fields of view structs
     included -- as (ordinal of the owning allocation, byte offset), so the text does not depend on where the allocator put things.

The test compares the SHA-256 and the line count of each text with EXPECTED.  EXPECTED is recorded from the PARENT of the commit
that introduced this module (EXPECTED_FROM: the tree in which all of this was `Engine`'s own), by running `record` below on a checkout
of it on an MI355X -- never from the code under test.  The recorder therefore uses only what both trees have: `Engine(...)`,
`eng.ops`, `eng._schedule()`, `Context.call`, `DeviceBuffer`.  Allocation sizes come from the library's `*_parts` / `*_floats`
entries, so the table belongs to that library too; the inputs' values do not matter to it (the launch list is static).

For a later change that moves a launch, a store or an allocation ON PURPOSE, record the table again from the commit that contains
that change once the parity tests have accepted it:

    python -c "import sys; sys.path[:0] = ['tests', '.']; import conftest, test_gpu_lowering_pinned as T; T.record(sys.stdout)"

A digest that changes without such a purpose is a bug; `text_of(ctx, name)` gives the text to diff against the parent's.
"""
import bisect
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from test_gpu_heads_pinned import hash32, hashed, one_hot
from tests.test_gpu_full_model import CW, SHAPE, build

pytestmark = pytest.mark.gpu

BATCH = 2
# read by the engine per pass: the text is the default path's
SWITCHES = ("SSDSEG_DET_SIDE", "SSDSEG_COPY2D_BATCH", "SSDSEG_COLSUM_DEFER", "SSDSEG_CONV3_PADFUSE", "SSDSEG_CONV3_SIDE")
# the attributes through which an op holds a Store, a Val or a list of Stores
STORE_FIELDS = ("image", "inp", "out", "out_val", "store", "a", "b", "outs", "logits", "prob", "probs", "boxes", "mask")


# ------------------------------------------------------------------------------------------------ observation
class Observer:
    """wraps DeviceBuffer creation and the context's `call` while installed; keeps every owned buffer alive so that no address is
    reused.  `call` is wrapped on the context object, not on the class: a test that spied on this context before (monkeypatch.setattr
    on the instance) leaves an instance attribute behind that would shadow a wrapper on the class, and the trace would stay empty."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.allocs = []          # (nbytes, dtype) by ordinal
        self.bases, self.spans = [], []      # sorted base addresses and (base, size, ordinal)
        self.keep = []
        self.trace = None         # list of lines while a pass is traced
        self.unresolved = 0

    def install(self):
        from ssdseglib import _hip as H
        self.H = H
        self._init, self._call, self._shadowed = H.DeviceBuffer.__init__, self.ctx.call, "call" in self.ctx.__dict__
        obs = self

        def init(buf, ctx, shape, dtype=np.float32, ptr=None, owner=None):
            obs._init(buf, ctx, shape, dtype, ptr=ptr, owner=owner)
            if ptr is None:
                i = bisect.bisect(obs.bases, buf.ptr)
                obs.bases.insert(i, buf.ptr)
                obs.spans.insert(i, (buf.ptr, max(buf.nbytes, 4), len(obs.allocs)))
                obs.allocs.append((buf.nbytes, str(buf.dtype)))
                obs.keep.append(buf)

        def call(name, *args):
            if obs.trace is not None:
                obs.trace.append(name + " " + " ".join(obs.arg(a) for a in args))
            return obs._call(name, *args)

        H.DeviceBuffer.__init__, self.ctx.call = init, call

    def remove(self):
        self.H.DeviceBuffer.__init__ = self._init
        if self._shadowed:
            self.ctx.call = self._call
        else:
            del self.ctx.call

    def where(self, ptr):
        if not ptr:
            return "null"
        i = bisect.bisect(self.bases, ptr) - 1
        if i >= 0:
            base, size, ordinal = self.spans[i]
            if ptr < base + size:
                return f"@{ordinal}+{ptr - base}"
        self.unresolved += 1
        return "@?"

    def arg(self, a):
        H = self.H
        if a is None:
            return "None"
        if isinstance(a, H.DeviceBuffer):
            return self.where(a.ptr)
        if isinstance(a, H.ViewStruct):
            return f"view({self.where(a.x)},{self.where(a.scale)},{self.where(a.shift)},{a.act})"
        if isinstance(a, H.GViewStruct):
            return "gview(" + ",".join(self.where(p) for p in (a.g, a.y, a.scale, a.shift, a.k1, a.k0)) + f",{a.act})"
        if isinstance(a, C.c_void_p):
            return self.where(a.value)
        if isinstance(a, C.Array):
            return "[" + ",".join(repr(float(x)) if isinstance(x, float) else repr(int(x)) for x in a) + "]"
        if isinstance(a, np.ndarray):
            return "[" + ",".join(repr(x) for x in a.reshape(-1).tolist()) + "]"
        if isinstance(a, C._SimpleCData):
            a = a.value
        if isinstance(a, (bool, int, np.integer)):
            return repr(int(a))
        if isinstance(a, (float, np.floating)):
            return repr(float(a))
        raise TypeError(f"argument of a kind the trace does not know: {type(a).__name__}")


def store_line(s):
    return (f"{s.name} ({s.n},{s.h},{s.w},{s.c}) ld={s.ld} coff={s.coff} parent={s.parent.name if s.parent is not None else None} "
            f"need_grad={s.need_grad} nparts={s.nparts}")


def op_lines(eng):
    from ssdseglib._ops import Store, Val
    out = []
    for op in eng.ops:
        out.append(f"op {type(op).__name__} {op.name!r} reach={sorted(op.reach)} fuse_input_bn={getattr(op, 'fuse_input_bn', None)} "
                   f"alias_a={getattr(op, 'alias_a', None)}")
        for field in STORE_FIELDS:
            x = getattr(op, field, None)
            for k, v in enumerate(x if isinstance(x, (list, tuple)) else (x,)):
                if isinstance(v, Val):
                    bn = f"{v.bn.layer.name}/{v.bn.act}" if v.bn is not None else None
                    out.append(f"  {field}[{k}] val act={v.act} affine={v.scale is not None} bn={bn} {store_line(v.store)}")
                elif isinstance(v, Store):
                    out.append(f"  {field}[{k}] {store_line(v)}")
    return out


def schedule_lines(eng):
    trunk, det, mask, join_before = eng._schedule()
    return ["trunk " + " | ".join(op.name for op in trunk), "det " + " | ".join(op.name for op in det), "mask " + " | ".join(op.name for op in mask),
            "join_before " + " | ".join(op.name for op in eng.ops if id(op) in join_before)]


# ------------------------------------------------------------------------------------------------ the cases
def images():
    return np.floor(hashed((BATCH,) + SHAPE, 31, 0.0, 256.0))


def targets_for(model):
    anchors = next(t.shape[1] for t in model.outputs if t.layer.name == "output-labels")
    labels = one_hot((BATCH, anchors), 32)
    positive = (labels[..., :1] == 0).astype(np.float32)
    return {"output-mask": one_hot((BATCH,) + SHAPE[:2], 33), "output-labels": labels, "output-boxes": hashed((BATCH, anchors, 4), 34, -2.0, 2.0) * positive}


def compile_reference_losses(model):
    import ssdseglib
    model.compile(optimizer=ssdseglib.optimizers.Adam(learning_rate=1e-3),
                  loss={'output-mask': ssdseglib.losses.cross_entropy(classes_weights=CW), 'output-labels': ssdseglib.losses.confidence_loss,
                        'output-boxes': ssdseglib.losses.localization_loss},
                  loss_weights={'output-mask': 1.0, 'output-labels': 1.0, 'output-boxes': 1.0})


def shufflenet_model():
    import ssdseglib
    from ssdseglib import _graph as K
    K.set_seed(3)
    d = np.zeros(4, np.float32)
    b = ssdseglib.models.ShuffleNetV2SsdSegBuilder(SHAPE, '1x', True, True, 6, 4, d, d, d, d, (0.1, 0.1, 0.2, 0.2))
    return b.get_model_for_training('deeplabv3plus', 'ssdlite', (3, 6, 12))


def training_engine(ctx, model):
    from ssdseglib import _engine as E
    compile_reference_losses(model)
    eng = E.Engine(model, BATCH, training=True, ctx=ctx)
    eng.configure_losses(model._compiled["loss"], model._compiled["loss_weights"])
    return eng


def case_mobilenet_training(ctx):
    model = build()[2]
    return model, training_engine(ctx, model), True


def case_shufflenet_training(ctx):
    model = shufflenet_model()
    return model, training_engine(ctx, model), True


def case_mobilenet_inference(ctx):
    from ssdseglib import _engine as E
    _, builder, model = build()
    inference = builder.get_model_for_inference(model_trained=model, max_number_of_boxes_per_class=4, max_number_of_boxes_per_sample=10,
                                                boxes_iou_threshold=0.3, labels_probability_threshold=0.26, suppress_background_boxes=False,
                                                use_segmentation_suppression=True)
    return inference, E.Engine(inference, BATCH, training=False, ctx=ctx), False


def case_mobilenet_eval(ctx):
    from ssdseglib import _engine as E
    model = build()[2]
    compile_reference_losses(model)
    before = E._default_ctx
    E.set_default_context(ctx)
    try:
        return model, E.eval_engine_for(model, BATCH), False
    finally:
        E.set_default_context(before)


CASES = {"mobilenetv2 training": case_mobilenet_training, "mobilenetv2 inference": case_mobilenet_inference,
         "shufflenetv2 1x training": case_shufflenet_training, "mobilenetv2 eval": case_mobilenet_eval}


def text_of(ctx, name):
    before = {k: os.environ.pop(k, None) for k in SWITCHES}
    obs = Observer(ctx)
    obs.install()
    try:
        model, eng, training = CASES[name](ctx)
        lines = [f"case {name}", f"allocations {len(obs.allocs)}"]
        lines += [f"alloc {i} {nbytes} {dtype}" for i, (nbytes, dtype) in enumerate(obs.allocs)]
        built = len(obs.allocs)
        lines += op_lines(eng)
        if training:
            lines += schedule_lines(eng)
        obs.trace = []
        if training:
            eng.train_step(images(), targets_for(model), optimizer=model._compiled["optimizer"])
        else:
            eng.set_input(images())
            if eng._loss_names:
                eng.set_targets(targets_for(model))
            eng.forward()
        ctx.sync()
        lines.append(f"calls {len(obs.trace)}")
        lines += obs.trace
        lines += [f"alloc-in-pass {i} {nbytes} {dtype}" for i, (nbytes, dtype) in enumerate(obs.allocs) if i >= built]
        lines.append(f"unresolved pointers {obs.unresolved}")
        return "\n".join(lines) + "\n"
    finally:
        obs.remove()
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest(), text.count("\n")


def record(out, keep_dir=None):
    """prints the table of this build (for EXPECTED: run it on the commit the table is to be taken from, see the module docstring);
    keep_dir: also leave each text there, to diff two trees"""
    from ssdseglib import _hip as H
    ctx = H.Context(0)
    out.write("EXPECTED = {\n")
    for name in CASES:
        text = text_of(ctx, name)
        if keep_dir:
            with open(os.path.join(keep_dir, name.replace(" ", "_") + ".txt"), "w") as f:
                f.write(text)
        out.write(f"    {name!r}: {digest(text)!r},\n")
    out.write("}\n")
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("name", list(CASES))
def test_lowering_allocations_ops_schedule_and_calls_are_pinned(ctx, name):
    text = text_of(ctx, name)
    assert "unresolved pointers 0\n" in text
    assert digest(text) == EXPECTED[name], name


def test_expected_table_is_not_empty():
    """the recorded table itself: one entry per case, and no text so short that a pass without calls could have made it"""
    assert set(EXPECTED) == set(CASES)
    assert all(len(sha) == 64 and lines > 500 for sha, lines in EXPECTED.values())


# Recorded with `record` above, one process, on an MI355X from a checkout of the commit named here (the parent of the commit that
# introduced this module).  {case: (SHA-256 of the text, its number of lines)}
EXPECTED_FROM = "d1c7ded4122c8103d3929d2402aca519438aa8d3"
EXPECTED = {
    'mobilenetv2 training': ('1992add9072beaf55381496b8bb53217a722121827df7d0dc659b9213fd95e66', 1622),
    'mobilenetv2 inference': ('65ba21824a6f6ada1f4a0bbbb462cfffa7da7665ac228576f42a7a5e39caa8c0', 1314),
    'shufflenetv2 1x training': ('4c82a53f5c9161acb476cd603edc28aa411fca10b4ccc9dad7a89ac6f5c31ae4', 2629),
    'mobilenetv2 eval': ('7b184830778eb80b908f50be932fa105b381db7eff9441197350008607bd4269', 1312),
}
