"""The loss and metric bindings without a device or a library: the real `_ops.MaskHeadOp` / `DetLossOp` and `_loss_bind` code on a
recording stub.  Pinned here: which C entry every loss takes and with which arguments (the launch table below, written down from
the code before the bindings moved out of the engine), that every `configure_losses` call rebuilds the binding state from its own
arguments alone, and that every error keeps its type and text and is raised before anything is bound."""
from types import SimpleNamespace

import numpy as np
import pytest

from ssdseglib import _loss_bind as LB
from ssdseglib import losses as LS
from ssdseglib import metrics as MT
from ssdseglib._ops import MaskHeadOp, Store, Val

BATCH, ANCHORS = 2, 10
H, W, C, FY, FX = 3, 4, 4, 4, 4                    # logits [2][3][4][4], up-sampled x(4, 4): 12 x 16 = 192 pixels
PIXELS = H * FY * W * FX
CW = [0.5, 1.0, 2.0, 1.5]
NAMES = ("output-mask", "output-labels", "output-boxes")
ONES = {n: 1.0 for n in NAMES}


class Buf:
    """what the ops need of a device buffer"""

    def __init__(self, shape, dtype=np.float32):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)

    def view(self, offset, shape, dtype=None):
        return Buf(shape, dtype or self.dtype)

    def reshape(self, shape):
        return Buf(shape, self.dtype)

    def zero_(self):
        return self

    upload = copy_from = lambda self, other: self


class Ctx:
    def __init__(self):
        self.calls = []

    def empty(self, shape, dtype=np.float32):
        return Buf(shape, dtype)

    zeros = empty

    def array(self, a, dtype=None):
        return Buf(np.shape(a), dtype or np.asarray(a).dtype)

    def call(self, name, *args):
        self.calls.append((name, args))


def stub_engine(training=True):
    eng = SimpleNamespace(ctx=Ctx(), batch=BATCH, training=training, stores=[], ops=[], loss_ops={}, loaders={"stale": object()}, vals={},
                          _loss_names=[], _metrics=[], _cur_reach=frozenset(), DET_OUTPUTS=frozenset(NAMES[1:]))

    def emit(op):                                   # as Engine._emit
        op.reach = eng._cur_reach
        eng.ops.append(op)
        return op

    eng._emit = emit
    mask_logits = Store(eng, BATCH, H, W, C, "mask-logits")
    det_logits, boxes = Store(eng, BATCH, ANCHORS, 1, 4, "logits"), Store(eng, BATCH, ANCHORS, 1, 4, "boxes")
    probs = Store(eng, BATCH, ANCHORS, 1, 4, "probs", need_grad=False)
    eng.stores += [mask_logits, det_logits, boxes, probs]
    head = eng.loss_ops[NAMES[0]] = eng._emit(MaskHeadOp(eng, Val(mask_logits), FY, FX, NAMES[0], None))      # no probability store
    outputs = [SimpleNamespace(layer=SimpleNamespace(name=n)) for n in NAMES]
    for t, v in zip(outputs, (Val(mask_logits, mask_head=head), Val(probs, logits=det_logits), Val(boxes, head_concat=True))):
        eng.vals[id(t)] = v
    eng.model = SimpleNamespace(outputs=outputs)
    eng.t = SimpleNamespace(head=head, mask_logits=mask_logits, det_logits=det_logits, probs=probs, boxes=boxes)
    return eng


def giou_loss(anchors=ANCHORS):
    v = np.linspace(0.1, 0.9, anchors)
    return LS.iou_localization_loss(v, v, v, v, (0.1, 0.1, 0.2, 0.2), kind="giou", smooth_l1_weight=0.75)


def bind(eng, mask=None, conf=None, loc=None, weights=ONES):
    LB.bind_losses(eng, {n: fn for n, fn in zip(NAMES, (mask, conf, loc)) if fn is not None}, weights)
    return eng


def step(eng):
    """forward then backward of the two loss ops -> the calls recorded"""
    del eng.ctx.calls[:]
    for op in eng.ops:
        op.fwd()
    for s in eng.stores:                            # as Engine._begin_backward
        s.gwritten = False
    for op in reversed(eng.ops):
        op.bwd()
    return list(eng.ctx.calls)


def check_call(got, name, *want):
    """buffers and host arrays by identity, numbers by value"""
    assert got[0] == name and len(got[1]) == len(want), (got[0], len(got[1]), name, len(want))
    for i, (a, w) in enumerate(zip(got[1], want)):
        assert a is w or (type(w) in (int, float) and type(a) is type(w) and a == w), (name, i, a, w)


# ------------------------------------------------------------------------------------------------------- a. the launch table
def head_args(eng):
    return (eng.t.mask_logits.buf, BATCH, H, W, C, FY, FX)


def test_cross_entropy_launches():
    eng = bind(stub_engine(), mask=LS.cross_entropy(CW))
    op = eng.t.head
    fwd, bwd = step(eng)
    g = eng.t.mask_logits.grad
    check_call(fwd, "ssdseg_mask_head_fwd", *head_args(eng), op.y_true, op.class_weights, None, op.loss)
    check_call(bwd, "ssdseg_mask_head_bwd", *head_args(eng), op.y_true, op.class_weights, 0.5, g)
    assert op.y_true.shape == (BATCH, H * FY, W * FX, C) and op.loss.shape == (BATCH,) and tuple(op.class_weights) == tuple(CW)
    (r,) = eng._loss_names
    assert r.target is op.y_true and r.loss is op.loss and r.weight == 1.0


@pytest.mark.parametrize("factory,flag", [(LS.dice, 0), (LS.dice_square, 1)])
def test_dice_launches(factory, flag):
    eng = bind(stub_engine(), mask=factory(CW))
    op = eng.t.head
    coef = op.loss_impl.coef
    fwd, bwd = step(eng)
    check_call(fwd, "ssdseg_mask_head_fwd_dice", *head_args(eng), op.y_true, op.class_weights, flag, None, op.loss, coef)
    check_call(bwd, "ssdseg_mask_head_bwd_dice", *head_args(eng), op.y_true, coef, flag, 0.5, eng.t.mask_logits.grad)
    assert coef.shape == (BATCH, 8) and fwd[1][-1] is bwd[1][8]


def test_bootstrapped_launches():
    eng = bind(stub_engine(), mask=LS.bootstrapped_cross_entropy(CW, 0.3))
    op = eng.t.head
    impl = op.loss_impl
    fwd, bwd = step(eng)
    check_call(fwd, "ssdseg_mask_head_fwd_bootstrap", *head_args(eng), op.y_true, op.class_weights, impl.keep, None, impl.pixel_loss, impl.thresh,
               impl.kept, op.loss)
    check_call(bwd, "ssdseg_mask_head_bwd_bootstrap", *head_args(eng), op.y_true, op.class_weights, impl.pixel_loss, impl.thresh, 0.5,
               eng.t.mask_logits.grad)
    assert fwd[1][11] is bwd[1][9] and fwd[1][12] is bwd[1][10]                     # pixel_loss, thresh: forward's are backward's
    assert impl.pixel_loss.shape == (BATCH, PIXELS) and impl.thresh.shape == (BATCH,)
    assert impl.kept.shape == (BATCH,) and impl.kept.dtype == np.int32
    assert impl.keep == LS.bootstrap_keep(0.3, PIXELS) == 58
    assert op.kind == "bootstrapped_cross_entropy" and op.keep == 58                # the op's read-only views of its variant
    assert op.pixel_loss is impl.pixel_loss and op.thresh is impl.thresh and op.kept is impl.kept


def test_no_loss_bound_is_the_plain_forward():
    eng = stub_engine(training=False)
    (fwd,) = step(eng)                                                              # bwd() records nothing
    check_call(fwd, "ssdseg_mask_head_fwd", *head_args(eng), None, None, None, None)


def det_ins(eng):
    det = eng.loss_ops["det"]
    return (det.y_labels, eng.t.probs.buf, det.y_boxes, eng.t.boxes.buf, BATCH, ANCHORS, 4)


def det_step(eng):
    """the detection op's calls of one step, and what they may write: the bindings' loss buffers and the two gradients"""
    calls = [c for c in step(eng) if "mask_head" not in c[0]]
    conf, loc = (next(r.loss for r in eng._loss_names if r.kind == k) for k in ("conf", "loc"))
    tr = eng.training
    return calls, conf, loc, eng.t.det_logits.grad if tr else None, eng.t.boxes.grad if tr else None


@pytest.mark.parametrize("training", [True, False])
def test_mined_launches(training):
    eng = bind(stub_engine(training), LS.cross_entropy(CW), LS.confidence_loss, LS.localization_loss)
    (call,), conf, loc, dlogits, dboxes = det_step(eng)
    check_call(call, "ssdseg_det_loss", *det_ins(eng), 0.5, conf, loc, dlogits, dboxes, None)
    det = eng.loss_ops["det"]
    assert det.y_labels.shape == (BATCH, ANCHORS, 4) and det.y_boxes.shape == (BATCH, ANCHORS, 4) and (dlogits is None) == (not training)

    bind(eng, LS.cross_entropy(CW), LS.confidence_loss, LS.localization_loss, {NAMES[2]: 2.0})
    (call,), conf, loc, dlogits, dboxes = det_step(eng)
    check_call(call, "ssdseg_det_loss_scaled", *det_ins(eng), 0.5, 1.0, conf, loc, dlogits, dboxes, None)


@pytest.mark.parametrize("training", [True, False])
def test_focal_launches(training):
    focal = LS.focal_confidence_loss((0.25, 1.0, 0.75, 0.5), 1.5)
    eng = bind(stub_engine(training), LS.cross_entropy(CW), focal, LS.localization_loss, {NAMES[2]: 2.0})
    (call,), conf, loc, dlogits, dboxes = det_step(eng)
    impl = eng.loss_ops["det"].conf_impl
    check_call(call, "ssdseg_det_loss_focal", *det_ins(eng), impl.alpha, 1.5, 0.5, 1.0, conf, loc, dlogits, dboxes)
    assert tuple(impl.alpha) == focal.alpha


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("w_conf", [1.0, 3.0])
def test_iou_localization_launches(training, w_conf):
    """the confidence entry without its localization half (the single-scale one whatever the weights), then the IoU entry"""
    giou = giou_loss()
    eng = bind(stub_engine(training), LS.cross_entropy(CW), LS.confidence_loss, giou, {NAMES[1]: w_conf, NAMES[2]: 3.0})
    (first, second), conf, loc, dlogits, dboxes = det_step(eng)
    det = eng.loss_ops["det"]
    assert det.loc is giou and det.loc_kind == 1 and det.kind == "mined"
    check_call(first, "ssdseg_det_loss", *det_ins(eng), w_conf / 2, conf, None, dlogits, None, None)
    check_call(second, "ssdseg_loc_loss_iou", det.y_boxes, eng.t.boxes.buf, giou.anchors_on(eng.ctx), giou._stds, BATCH, ANCHORS, 1, 0.75, 1.5,
               loc, dboxes)

    bind(eng, LS.cross_entropy(CW), LS.focal_confidence_loss(), giou, {NAMES[2]: 3.0})
    (first, second), conf, loc, dlogits, dboxes = det_step(eng)
    check_call(first, "ssdseg_det_loss_focal", *det_ins(eng), det.conf_impl.alpha, 2.0, 0.5, 1.5, conf, None, dlogits, None)
    check_call(second, "ssdseg_loc_loss_iou", det.y_boxes, eng.t.boxes.buf, giou.anchors_on(eng.ctx), giou._stds, BATCH, ANCHORS, 1, 0.75, 1.5,
               loc, dboxes)


# ------------------------------------------------------------------------------------------------------------ b. bind_losses
def test_bind_losses_on_the_stub_engine():
    eng = stub_engine()
    weights = {NAMES[0]: 0.5, NAMES[1]: 2.0, NAMES[2]: 3.0}
    bind(eng, LS.cross_entropy(CW), LS.confidence_loss, LS.localization_loss, weights)
    det = eng.loss_ops["det"]
    targets = (det.y_labels, det.y_boxes)
    assert [(r.name, r.kind) for r in eng._loss_names] == list(zip(NAMES, ("mask", "conf", "loc")))
    assert [r.weight for r in eng._loss_names] == [0.5, 2.0, 3.0] and (det.w_conf, det.w_loc) == (2.0, 3.0)
    assert [tuple(r) for r in eng._loss_names] == [(NAMES[0], eng.t.head, "mask"), (NAMES[1], det, "conf"), (NAMES[2], det, "loc")]
    assert eng.loaders == {} and det.reach == eng.DET_OUTPUTS
    eng.loaders["stale"] = object()
    bind(eng, LS.dice(CW), LS.focal_confidence_loss(), giou_loss(), weights)
    assert eng.ops.count(det) == 1 and len(eng.ops) == 2 and eng.loss_ops["det"] is det          # emitted once, kept
    assert (det.y_labels, det.y_boxes) == targets and eng.loaders == {}
    assert [r.target for r in eng._loss_names][1:] == list(targets)


# ------------------------------------------------------------------------------------------------------------- c. re-binding
def test_focal_then_mined_leaves_no_focal_state():
    eng = bind(stub_engine(), LS.cross_entropy(CW), LS.focal_confidence_loss((0.25, 1.0, 0.75, 0.5), 1.5), giou_loss())
    bind(eng, LS.cross_entropy(CW), LS.confidence_loss, LS.localization_loss)
    (call,), conf, loc, dlogits, dboxes = det_step(eng)
    check_call(call, "ssdseg_det_loss", *det_ins(eng), 0.5, conf, loc, dlogits, dboxes, None)
    det = eng.loss_ops["det"]
    assert det.kind == "mined" and det.loc is None and det.loc_kind == 0 and not hasattr(det.conf_impl, "alpha")


def test_bootstrapped_then_cross_entropy_leaves_no_bootstrap_state():
    eng = bind(stub_engine(), mask=LS.bootstrapped_cross_entropy(CW, 0.25))
    op = eng.t.head
    old = op.loss_impl
    bind(eng, mask=LS.cross_entropy(CW))
    reachable = list(vars(op).values()) + list(vars(op.loss_impl).values())
    assert not any(x is y for x in reachable for y in (old, old.pixel_loss, old.thresh, old.kept))
    assert op.loss_impl.kind == "cross_entropy" and not any(hasattr(op.loss_impl, a) for a in ("keep", "pixel_loss", "thresh", "kept"))
    assert op.kind == "cross_entropy" and op.keep == 0 and op.pixel_loss is None and op.thresh is None and op.kept is None
    assert [c[0] for c in step(eng)] == ["ssdseg_mask_head_fwd", "ssdseg_mask_head_bwd"]


def test_a_weight_or_loss_that_is_not_named_leaves_nothing_behind():
    three = (LS.cross_entropy(CW), LS.confidence_loss, LS.localization_loss)
    eng = bind(stub_engine(), *three, {NAMES[1]: 1.5, NAMES[2]: 1.5})
    (call,), *_ = det_step(eng)
    assert call[1][7] == 0.75
    bind(eng, *three, {})
    (call,), conf, loc, dlogits, dboxes = det_step(eng)
    check_call(call, "ssdseg_det_loss", *det_ins(eng), 0.5, conf, loc, dlogits, dboxes, None)
    bind(eng, LS.cross_entropy(CW), LS.focal_confidence_loss(), giou_loss(), {NAMES[1]: 4.0, NAMES[2]: 4.0})
    bind(eng, mask=None, conf=None, loc=LS.localization_loss, weights={})
    det, op = eng.loss_ops["det"], eng.t.head
    assert [r.kind for r in eng._loss_names] == ["loc"] and (det.kind, det.w_conf, det.w_loc) == ("mined", 1.0, 1.0)
    assert op.loss_impl is None and op.y_true is None and op.loss is None
    calls = step(eng)
    check_call(calls[0], "ssdseg_mask_head_fwd", *head_args(eng), None, None, None, None)
    assert [c[0] for c in calls] == ["ssdseg_mask_head_fwd", "ssdseg_det_loss"]


# ------------------------------------------------------------------------------------------------------------------ d. errors
def tversky(y_true, y_pred):
    raise AssertionError("never called")


tversky.loss_kind, tversky.classes_weights = "tversky", CW
MASK_HEAD_TEXT = ("loss for output output-mask: the mask head trains with ssdseglib.losses.cross_entropy / dice / dice_square / "
                  "bootstrapped_cross_entropy")
LOSS_ERRORS = [
    (dict(conf=lambda y, p: 0.0), NotImplementedError, "loss for output output-labels: only the ssdseglib.losses functions are supported"),
    (dict(mask=tversky), NotImplementedError, MASK_HEAD_TEXT),
    (dict(mask=LS.confidence_loss), NotImplementedError, MASK_HEAD_TEXT),
    (dict(conf=giou_loss()), ValueError, "loss iou_localization_loss does not fit output output-labels: it takes the box offsets"),
    (dict(loc=giou_loss(ANCHORS - 3)), ValueError, "loss iou_localization_loss: 7 default boxes, output output-boxes has 10 anchors"),
    (dict(loc=LS.focal_confidence_loss()), ValueError,
     "loss focal_confidence_loss does not fit output output-boxes: it takes the class probabilities"),
]


def snapshot(eng):
    return (eng._loss_names, list(eng._loss_names), eng._metrics, list(eng._metrics), list(eng.ops), dict(eng.loss_ops), dict(eng.loaders),
            [dict(vars(op)) for op in eng.ops])


@pytest.mark.parametrize("first", ["nothing bound yet", "bound before"])
@pytest.mark.parametrize("bad,exc,text", LOSS_ERRORS)
def test_loss_errors_come_before_anything_is_bound(first, bad, exc, text):
    eng = stub_engine()
    good = dict(mask=LS.dice(CW), conf=LS.confidence_loss, loc=LS.localization_loss)
    if first == "bound before":
        bind(eng, **good)
        eng.loaders["kept"] = object()
    before = snapshot(eng)
    with pytest.raises(exc) as err:
        bind(eng, **{**good, **bad})
    assert str(err.value) == text
    after = snapshot(eng)
    assert after == before and after[0] is before[0] and after[2] is before[2]


def test_metric_errors_come_before_anything_is_bound():
    eng = bind(stub_engine(), mask=LS.cross_entropy(CW), loc=LS.localization_loss)
    LB.bind_metrics(eng, {NAMES[0]: MT.jaccard_iou_segmentation_masks(CW)})
    before = snapshot(eng)
    cases = [({NAMES[1]: MT.categorical_accuracy(CW)}, NotImplementedError,
              "metric for output output-labels needs a compiled loss on the same output (it shares its target buffer)"),
             ({NAMES[2]: [MT.categorical_accuracy(CW)]}, ValueError, "metric categorical_accuracy_metric does not fit output output-boxes"),
             ({NAMES[0]: max}, NotImplementedError, "metric for output output-mask: only the ssdseglib.metrics factories are supported")]
    for bad, exc, text in cases:
        with pytest.raises(exc) as err:
            LB.bind_metrics(eng, {NAMES[0]: MT.jaccard_iou_segmentation_masks(CW), **bad})
        assert str(err.value) == text
        after = snapshot(eng)
        assert after == before and after[2] is before[2]


# ----------------------------------------------------------------------------------------------------------------- e. metrics
def test_metric_launches():
    eng = bind(stub_engine(training=False), LS.cross_entropy(CW), LS.confidence_loss, LS.localization_loss)
    v = np.linspace(0.1, 0.9, ANCHORS)
    fns = (MT.jaccard_iou_segmentation_masks(CW), MT.categorical_accuracy(CW), MT.jaccard_iou_bounding_boxes(v, v, v, v, (0.1, 0.1, 0.2, 0.2)))
    LB.bind_metrics(eng, {NAMES[0]: fns[0], NAMES[1]: [fns[1]], NAMES[2]: (fns[2],)})
    assert [m[0] for m in eng._metrics] == ["output-mask_jaccard_iou_segmentation_masks_metric", "output-labels_categorical_accuracy_metric",
                                            "output-boxes_jaccard_iou_bounding_boxes_metric"]
    assert [m[1] for m in eng._metrics] == ["mask_iou", "label_accuracy", "box_iou"] and all(m[4].shape == (BATCH,) for m in eng._metrics)
    outs = [m[4] for m in eng._metrics]
    del eng.ctx.calls[:]
    LB.launch_metrics(eng)
    mask, labels, boxes = eng.ctx.calls
    op, det = eng.t.head, eng.loss_ops["det"]
    check_call(mask, "ssdseg_metric_mask_iou", *head_args(eng), 1, op.y_true, fns[0]._cw, outs[0])
    check_call(labels, "ssdseg_metric_label_accuracy", det.y_labels, eng.t.probs.buf, BATCH, ANCHORS, 4, fns[1]._cw, outs[1])
    check_call(boxes, "ssdseg_metric_box_iou", det.y_boxes, eng.t.boxes.buf, fns[2].anchors_on(eng.ctx), fns[2]._stds, BATCH, ANCHORS, outs[2])


def test_engine_reexports_the_binding():
    from ssdseglib import _engine
    assert _engine.LossBinding is LB.LossBinding
    r = LB.LossBinding("output-mask", None, "mask", None, None, 1.0)
    assert tuple(r) == ("output-mask", None, "mask")
