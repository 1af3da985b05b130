"""CPU: the parts of the lowering that need no device -- the branch schedule on hand-built op lists, the concat placement plan of
the two backbones, and the import direction of the new modules."""
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

SHAPE = (96, 128, 3)
FMAPS = ((6, 8), (3, 4), (2, 2), (1, 1))
STDS = (0.1, 0.1, 0.2, 0.2)


def mobilenet_model():
    import ssdseglib
    from ssdseglib import _graph as K
    K.set_seed(11)
    boxes = ssdseglib.boxes.DefaultBoundingBoxes(feature_maps_shapes=FMAPS, centers_padding_from_borders_percentage=0.05, boxes_scales=(0.15, 0.95))
    boxes.rescale_boxes_coordinates(SHAPE[:2])
    builder = ssdseglib.models.MobileNetV2SsdSegBuilder(
        SHAPE, [6, 6, 6, 6], 4, boxes.get_boxes_coordinates_center_x('ssd'), boxes.get_boxes_coordinates_center_y('ssd'),
        boxes.get_boxes_coordinates_width('ssd'), boxes.get_boxes_coordinates_height('ssd'), STDS)
    return builder.get_model_for_training('deeplabv3plus', 'ssdlite', (3, 6, 12))


def shufflenet_model():
    import ssdseglib
    from ssdseglib import _graph as K
    K.set_seed(3)
    d = np.zeros(4, np.float32)
    b = ssdseglib.models.ShuffleNetV2SsdSegBuilder(SHAPE, '1x', True, True, 6, 4, d, d, d, d, STDS)
    return b.get_model_for_training('deeplabv3plus', 'ssdlite', (3, 6, 12))


# ------------------------------------------------------------------------------------------------ plan_branches on hand-built ops
MASK, LABELS, BOXES = "output-mask", "output-labels", "output-boxes"
DET = frozenset((LABELS, BOXES))
ALL = frozenset((MASK, LABELS, BOXES))


def store(name, parent=None):
    """a Store that allocates nothing: `buf` is given"""
    from ssdseglib._ops import Store
    eng = SimpleNamespace(stores=[])
    return Store(eng, 1, 2, 2, 4, name, buf=object(), parent=parent)


def op(name, reach, *stores):
    """a plain object with what plan_branches reads: `reach` and attributes that hold Stores"""
    return SimpleNamespace(name=name, reach=frozenset(reach), **{f"s{i}": s for i, s in enumerate(stores)})


def plan(ops):
    from ssdseglib._branches import plan_branches
    trunk, det, mask, join_before = plan_branches(ops, DET)
    return ([o.name for o in trunk], [o.name for o in det], [o.name for o in mask], {o.name for o in ops if id(o) in join_before})


def serial(ops):
    return [o.name for o in ops], [], [], set()


def test_no_detection_only_op_is_serial():
    x, y, z = store("x"), store("y"), store("z")
    ops = [op("a", ALL, x, y), op("m", {MASK}, y, z)]         # a mask branch alone: nothing to run beside it
    assert plan(ops) == serial(ops)
    ops = [op("a", ALL, x, y), op("d", DET, y, z)]            # and a detection branch alone
    assert plan(ops) == serial(ops)


def test_trunk_and_two_branches_fork():
    """trunk a, b; detection d1, d2 (d2 reaches only the boxes: still a subset of the detection outputs); mask m1, m2.  The tap `t`
    is read by d1 and m1: m1 comes first in layer order, so d1 is not demoted (it is not ahead of a mask reader), rule (1) has no
    demoted op to check, and rule (2) holds: on `t` the trunk op b (1) precedes both branch ops and the mask op (2) the detection
    op (3).  join_before: m1 shares `t` with the detection branch, m2 shares nothing with it."""
    x, t, dm, dd, m2s, d2s = (store(n) for n in ("x", "t", "dm", "dd", "m2s", "d2s"))
    ops = [op("a", ALL, x), op("b", ALL, x, t), op("m1", {MASK}, t, dm), op("d1", DET, t, dd), op("m2", {MASK}, dm, m2s), op("d2", {BOXES}, dd, d2s)]
    assert plan(ops) == (["a", "b"], ["d1", "d2"], ["m1", "m2"], {"m1"})


def test_a_store_is_touched_through_its_parent_too():
    """the detection op writes a slice of the buffer the mask op reads whole: they share the parent, so the mask op joins"""
    x, whole = store("x"), store("whole")
    part = store("part", parent=whole)
    ops = [op("a", ALL, x), op("m0", {MASK}, x, whole), op("d1", DET, x, part), op("m1", {MASK}, whole)]
    # d1 (2) is ahead of m1 (3) on `whole`: demoted.  No detection op is left: serial
    assert plan(ops) == serial(ops)
    ops = [op("a", ALL, x), op("m1", {MASK}, x, whole), op("d1", DET, x, part)]
    # nothing of the mask branch behind d1: it stays a detection op; trunk a (0) precedes both on `x`, mask (1) precedes detection (2)
    assert plan(ops) == (["a"], ["d1"], ["m1"], {"m1"})


def test_early_detection_op_is_demoted_to_the_trunk():
    """d0 reads the tap `t` BEFORE the mask reader m1: it is the last contributor to dL/dt and stays with the trunk, at its place in
    layer order.  Rule (1): no detection op ahead of d0.  Rule (2): on `t` the trunk ops b (1), d0 (2) precede the only branch op
    m1 (3); on `u` (d0 -> d1) the trunk op d0 (2) precedes d1 (4).  m1 shares no store with the detection branch {d1}: no join."""
    x, t, u, dm, dd = (store(n) for n in ("x", "t", "u", "dm", "dd"))
    ops = [op("a", ALL, x), op("b", ALL, x, t), op("d0", DET, t, u), op("m1", {MASK}, t, dm), op("d1", DET, u, dd)]
    assert plan(ops) == (["a", "b", "d0"], ["d1"], ["m1"], set())


def test_rule_1_demoted_op_behind_a_detection_op_on_a_shared_store_is_serial():
    """d1 is demoted (it reads `t` ahead of the mask reader m1) but also reads `u`, which the detection op d0 ahead of it wrote:
    before the fork it would read what the side stream has not produced"""
    x, t, u, dm, dd = (store(n) for n in ("x", "t", "u", "dm", "dd"))
    ops = [op("a", ALL, x, t), op("d0", DET, x, u), op("d1", DET, u, t, dd), op("m1", {MASK}, t, dm)]
    assert plan(ops) == serial(ops)


def test_rule_2_trunk_op_behind_a_branch_op_on_a_shared_store_is_serial():
    """the trunk op c (2) touches `t` after the mask op m1 (1) did: the backward order mask, trunk would no longer be the reverse
    layer order on `t`"""
    x, t, dm, dd = (store(n) for n in ("x", "t", "dm", "dd"))
    ops = [op("a", ALL, x, t), op("m1", {MASK}, t, dm), op("c", ALL, t, x), op("d1", DET, x, dd)]
    assert plan(ops) == serial(ops)


def test_rule_2_mask_op_behind_a_detection_op_on_a_shared_store_is_serial():
    """A detection op ahead of a mask op on a shared store is always demoted (that is the demotion's own condition), so the order
    mask-before-detection of rule (2) can only be broken through what the demotion leaves behind.  With nothing else in the detection
    branch the plan is serial because the branch is empty.  With a mask op on the store BEFORE it as well (m0, d1, m1 on `t`), the
    demoted d1 (2) is a trunk op behind the first branch op on `t` (m0, 1): rule (2), serial -- although d2 would keep the detection
    branch alive."""
    x, t, u, dm, dm2, dd = (store(n) for n in ("x", "t", "u", "dm", "dm2", "dd"))
    ops = [op("a", ALL, x, t), op("d1", DET, t, dd), op("m1", {MASK}, t, dm)]
    assert plan(ops) == serial(ops)
    ops = [op("a", ALL, x, t), op("m0", {MASK}, t, dm), op("d1", DET, t, u), op("m1", {MASK}, t, dm2), op("d2", DET, u, dd)]
    assert plan(ops) == serial(ops)
    # control: without m0 the same list forks, d1 with the trunk
    ops = [o for o in ops if o.name != "m0"]
    assert plan(ops) == (["a", "d1"], ["d2"], ["m1"], set())


# ------------------------------------------------------------------------------------------------ the concat placement plan
# {producer layer: (concat layer, channel offset)} of the two 96x128 training models, recorded from PLACEMENT_FROM (the parent of the
# commit that introduced `_lowering`) by calling its Engine._plan_concats on a stand-in object that has only `.model`
PLACEMENT_FROM = "d1c7ded4122c8103d3929d2402aca519438aa8d3"
DEEPLAB_PLACEMENT = {
    'mask-encoder-aspp-pointwise-conv': ('mask-encoder-concat', 0),
    'mask-encoder-aspp-atrous1-sepconv': ('mask-encoder-concat', 256),
    'mask-encoder-aspp-atrous2-sepconv': ('mask-encoder-concat', 512),
    'mask-encoder-aspp-atrous3-sepconv': ('mask-encoder-concat', 768),
    'mask-encoder-pooling-upsampling': ('mask-encoder-concat', 1024),
    'mask-decoder-upsampling-encoder-output': ('mask-decoder-concat', 0),
    'mask-decoder-backbone-conv': ('mask-decoder-concat', 256),
}
SHUFFLENET_PLACEMENT = {
    'backbone-stage2-downblock-branch-left-conv2': ('backbone-stage2-downblock--concat', 0),
    'backbone-stage2-downblock-branch-right-conv3': ('backbone-stage2-downblock--concat', 60),
    'backbone-stage3-downblock-branch-left-conv2': ('backbone-stage3-downblock--concat', 0),
    'backbone-stage3-downblock-branch-right-conv3': ('backbone-stage3-downblock--concat', 116),
    'backbone-stage4-downblock-branch-left-conv2': ('backbone-stage4-downblock--concat', 0),
    'backbone-stage4-downblock-branch-right-conv3': ('backbone-stage4-downblock--concat', 232),
    **DEEPLAB_PLACEMENT,
}


def placement_of(model):
    from ssdseglib import _lowering as LW
    placement = LW.plan_concats(model, LW.consumers(model), {id(t) for t in model.outputs})
    names = {id(l): l.name for l in model.layers}
    return {names[lid]: (concat.name, off) for lid, (concat, off) in placement.items()}


def test_concat_placement_mobilenetv2():
    assert placement_of(mobilenet_model()) == DEEPLAB_PLACEMENT


def test_concat_placement_shufflenetv2_1x():
    assert placement_of(shufflenet_model()) == SHUFFLENET_PLACEMENT


def test_consumer_predicates():
    """the two questions the fusion rules ask: the block-13 expansion's BatchNorm+ReLU6 output feeds block 13's depthwise conv first and
    the ASPP behind it -- first consumer, not sole consumer; block 1's is read by its depthwise conv alone"""
    from ssdseglib import _lowering as LW
    model = mobilenet_model()
    cons, outs = LW.consumers(model), {id(t) for t in model.outputs}
    tap = model.get_layer('backbone-block13-expand-relu6').outputs[0]
    dw13 = model.get_layer('backbone-block13-depthwise-conv')
    assert len(cons[id(tap)]) > 1 and LW.first_consumer(cons, tap, dw13) and not LW.sole_consumer(cons, outs, tap)
    assert not any(LW.first_consumer(cons, tap, l) for l in cons[id(tap)][1:])
    plain = model.get_layer('backbone-block1-expand-relu6').outputs[0]
    assert LW.sole_consumer(cons, outs, plain) and LW.first_consumer(cons, plain, model.get_layer('backbone-block1-depthwise-conv'))
    assert not any(LW.sole_consumer(cons, outs, t) for t in model.outputs)


# ------------------------------------------------------------------------------------------------ import direction
def test_lowering_and_branches_do_not_import_the_engine():
    code = ("import sys; sys.path[:0] = %r; import ssdseglib._lowering, ssdseglib._branches; "
            "assert 'ssdseglib._engine' not in sys.modules, 'the lowering must not import the engine'") % (sys.path,)
    subprocess.run([sys.executable, "-c", code], check=True)
