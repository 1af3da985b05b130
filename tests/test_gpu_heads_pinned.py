"""GPU: what the pooling / resize / mask-head / SSD-tail / metric entry points launch and compute -- pinned, bit for bit.

csrc/resize.hip, csrc/mask_head.hip and csrc/heads.hip write each piece of their kernel arithmetic once: the four-corner blend, the
output window of an input pixel, the softmax and the 256-thread tree sum in csrc/lerp_softmax.h, dz of a full-resolution pixel and
the eight per-image sums in csrc/mask_head.hip.  The parity tests hold these kernels to a tolerance against the oracle; this module
holds them to the exact bits of the code they were carved out of.  Every case makes its calls with the timing registry on and
compares two things with the committed table EXPECTED: the {kernel symbol: launches} map the calls leave, and a SHA-256 digest of
the raw bytes of each output.

The table is recorded from the PARENT of the commit that introduced this module (EXPECTED_FROM: the tree in which all of this was
one unit, csrc/heads.hip), by running `observe` below over CASES on a checkout of it on an MI355X, ROCm as named by EXPECTED_ROCM
-- never from the code under test.  The inputs are built from integer arithmetic alone (a multiplicative hash of the element index
mapped to a float range, one-hot targets and probabilities from the same hash), so the table does not depend on a random generator
or on the NumPy version.  Device-side expf / logf are part of what is pinned: the table belongs to that ROCm version.

For a later kernel change: whenever a kernel of these three units is changed ON PURPOSE (another summation order, another
expression), the digests of the cases that reach it change, and the table has to be recorded again -- check out the commit before
the change stops being bit-compatible, build, and run

    python -c "import sys; sys.path[:0] = ['tests', '.']; import test_gpu_heads_pinned as T; T.record(sys.stdout)"

on the GPU, then replace EXPECTED (and EXPECTED_FROM / EXPECTED_ROCM) with what it prints, after the parity tests have accepted the
new kernel.  A digest that changes without such a purpose is a bug.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU6 = 0, 2
CW = (0.05, 0.575, 0.135, 0.24)
STDS = (0.1, 0.1, 0.2, 0.2)


# ------------------------------------------------------------------------------------------------ inputs from integer arithmetic
def hash32(count, seed):
    """uint64 array of `count` 32-bit hashes of the element index (multiply, xor-shift, multiply, xor-shift; all mod 2^32)"""
    m = np.uint64(0xFFFFFFFF)
    h = (np.arange(count, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed * 40503 + 12345)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & m
    h ^= h >> np.uint64(16)
    return h


def hashed(shape, seed, lo, hi):
    """float32 values in [lo, hi): the top 24 bits of the hash, scaled in float64 (exact), rounded once"""
    h = hash32(int(np.prod(shape)), seed) >> np.uint64(8)
    return (lo + (hi - lo) * (h.astype(np.float64) / 16777216.0)).astype(np.float32).reshape(shape)


def one_hot(shape, seed):
    """float32 one-hot rows of depth 4, shape + (4,)"""
    cls = (hash32(int(np.prod(shape)), seed) >> np.uint64(20)) % np.uint64(4)
    return np.eye(4, dtype=np.float32)[cls.astype(np.int64)].reshape(tuple(shape) + (4,))


def probabilities(shape, seed):
    """float32 rows of depth 4 that sum to 1 up to rounding: four hashed integers in [1, 64] over their sum (no exp)"""
    a = ((hash32(int(np.prod(shape)) * 4, seed) >> np.uint64(12)) % np.uint64(64) + np.uint64(1)).astype(np.float64).reshape(-1, 4)
    return (a / a.sum(axis=1, keepdims=True)).astype(np.float32).reshape(tuple(shape) + (4,))


def c4(values):
    return (C.c_float * 4)(*values)


# ------------------------------------------------------------------------------------------------ the cases
# Each case: (name, environment switches, function(ctx) -> {output name: ndarray}).  Output buffers start as zeros (or as a hashed
# base where the call accumulates), so the bytes a call must leave alone are pinned with those it writes.
CASES = []


def case(name, env=None):
    def add(fn):
        CASES.append((name, dict(env or {}), fn))
        return fn
    return add


GATHER_RESIZE = {"SSDSEG_BILINEAR": "gather"}
GATHER_MASK = {"SSDSEG_MASK_BWD": "gather"}


def plain_view(x):
    from ssdseglib import _hip as H
    return H.view(x)


def affine_view(ctx, x, c, seed):
    from ssdseglib import _hip as H
    return H.view(x, ctx.array(hashed((c,), seed + 1, 0.5, 1.5)), ctx.array(hashed((c,), seed + 2, -1.0, 3.0)), ACT_RELU6)


def add_gap_cases():
    for n, hw, c, affine in ((2, 63, 8, True), (3, 1200, 576, True), (3, 1200, 576, False)):      # one launch; 16 chunks + chunk_sum
        @case(f"gap_fwd n{n} hw{hw} c{c} {'affine+relu6' if affine else 'identity'}")
        def _(ctx, n=n, hw=hw, c=c, affine=affine):
            x = ctx.array(hashed((n, hw, c), 1, -4.0, 4.0))
            out = ctx.zeros((n, c))
            ctx.call("ssdseg_gap_fwd", affine_view(ctx, x, c, 10) if affine else plain_view(x), out, n, hw, c)
            return {"out": out.download()}
    for acc in (0, 1):
        @case(f"gap_bwd n3 hw1200 c16 acc{acc}")
        def _(ctx, acc=acc):
            n, hw, c = 3, 1200, 16
            dx = ctx.array(hashed((n, hw, c), 3, -1.0, 1.0))
            ctx.call("ssdseg_gap_bwd", ctx.array(hashed((n, c), 2, -2.0, 2.0)), dx, n, hw, c, acc)
            return {"dx": dx.download()}


BILINEAR_SHAPES = [(2, 6, 8, 16, 4, 4), (2, 5, 7, 8, 4, 4), (3, 2, 1, 72, 4, 4), (1, 5, 7, 8, 2, 8), (1, 3, 3, 4, 1, 1)]


def add_bilinear_cases():
    for n, h, w, c, fy, fx in BILINEAR_SHAPES:
        for env in (({}, GATHER_RESIZE) if (fy, fx) == (4, 4) else ({},)):
            @case(f"bilinear n{n} h{h} w{w} c{c} x{fy}x{fx}" + (" gather" if env else ""), env)
            def _(ctx, n=n, h=h, w=w, c=c, fy=fy, fx=fx):
                x = ctx.array(hashed((n, h, w, c), 4, -4.0, 4.0))
                out = ctx.zeros((n, h * fy, w * fx, c))
                ctx.call("ssdseg_bilinear_fwd", affine_view(ctx, x, c, 20), c, out, c, n, h, w, c, fy, fx)
                g = ctx.array(hashed((n, h * fy, w * fx, c), 5, -1.0, 1.0))
                dx = ctx.zeros((n, h, w, c))
                ctx.call("ssdseg_bilinear_bwd", g, c, dx, c, n, h, w, c, fy, fx, 0)
                return {"out": out.download(), "dx": dx.download()}
    for acc in (0, 1):
        @case(f"bilinear_bwd pixel sum n2 c256 x30x40 acc{acc}")
        def _(ctx, acc=acc):
            n, c, fy, fx = 2, 256, 30, 40
            g = ctx.array(hashed((n, fy, fx, c), 6, -1.0, 1.0))
            dx = ctx.array(hashed((n, 1, 1, c), 7, -1.0, 1.0))
            ctx.call("ssdseg_bilinear_bwd", g, c, dx, c, n, 1, 1, c, fy, fx, acc)
            return {"dx": dx.download()}
    for env in ({}, GATHER_RESIZE):
        @case("bilinear wide rows and padded n2 h5 w7 c8 x4x4" + (" gather" if env else ""), env)
        def _(ctx):
            n, h, w, c, f, ld = 2, 5, 7, 8, 4, 16
            x = ctx.array(hashed((n * h * w, ld), 8, -4.0, 4.0))                 # the slice [4, 4 + c) of rows of ld floats
            v = affine_view(ctx, x.view(4, (x.size - 4,)), c, 30)
            out = ctx.zeros((n * h * f * w * f, ld))
            ctx.call("ssdseg_bilinear_fwd", v, ld, out.view(4, (out.size - 4,)), ld, n, h, w, c, f, f)
            padded = ctx.zeros((n, h * f + 2, w * f + 2, ld))
            ctx.call("ssdseg_bilinear_fwd_padded", v, ld, padded, ld, n, h, w, c, f, f)
            g = ctx.array(hashed((n * h * f * w * f, ld), 9, -1.0, 1.0))
            dx = ctx.zeros((n * h * w, ld))
            ctx.call("ssdseg_bilinear_bwd", g.view(4, (g.size - 4,)), ld, dx.view(4, (dx.size - 4,)), ld, n, h, w, c, f, f, 0)
            return {"out": out.download(), "padded": padded.download(), "dx": dx.download()}


MASK_SHAPES = [(n, h, w, f, f) for f in (4, 8) for n, h, w in ((2, 12, 16), (1, 17, 35), (3, 5, 3))] + [(1, 5, 7, 2, 8)]


def add_mask_cases():
    for n, h, w, fy, fx in MASK_SHAPES:
        tag = f"n{n} h{h} w{w} x{fy}x{fx}"

        def inputs(ctx, n=n, h=h, w=w, fy=fy, fx=fx):
            return ctx.array(hashed((n, h, w, 4), 11, -4.0, 4.0)), ctx.array(one_hot((n, h * fy, w * fx), 12))

        @case(f"mask_head_fwd {tag}")
        def _(ctx, n=n, h=h, w=w, fy=fy, fx=fx, inputs=inputs):
            logits, y = inputs(ctx)
            shape = (n, h * fy, w * fx, 4)
            prob, loss, prob_only, loss_only = ctx.zeros(shape), ctx.zeros((n,)), ctx.zeros(shape), ctx.zeros((n,))
            ctx.call("ssdseg_mask_head_fwd", logits, n, h, w, 4, fy, fx, y, c4(CW), prob, loss)
            ctx.call("ssdseg_mask_head_fwd", logits, n, h, w, 4, fy, fx, None, None, prob_only, None)
            ctx.call("ssdseg_mask_head_fwd", logits, n, h, w, 4, fy, fx, y, c4(CW), None, loss_only)
            return {"prob": prob.download(), "loss": loss.download(), "prob_only": prob_only.download(), "loss_only": loss_only.download()}

        for env in ({}, GATHER_MASK):
            @case(f"mask_head_bwd {tag}" + (" gather" if env else ""), env)
            def _(ctx, n=n, h=h, w=w, fy=fy, fx=fx, inputs=inputs):
                logits, y = inputs(ctx)
                g = ctx.zeros((n, h, w, 4))
                ctx.call("ssdseg_mask_head_bwd", logits, n, h, w, 4, fy, fx, y, c4(CW), 0.5, g)
                return {"dlogits": g.download()}


def add_dice_cases():
    for n, h, w in ((2, 6, 8), (3, 30, 40)):                 # one partial block per image; ten
        for squared in (0, 1):
            tag = f"n{n} h{h} w{w} x4x4 squared{squared}"

            def inputs(ctx, n=n, h=h, w=w):
                return ctx.array(hashed((n, h, w, 4), 13, -4.0, 4.0)), ctx.array(one_hot((n, h * 4, w * 4), 14))

            @case(f"mask_head_fwd_dice {tag}")
            def _(ctx, n=n, h=h, w=w, squared=squared, inputs=inputs):
                logits, y = inputs(ctx)
                prob, loss, coef, loss2, coef2 = ctx.zeros((n, h * 4, w * 4, 4)), ctx.zeros((n,)), ctx.zeros((n, 8)), ctx.zeros((n,)), ctx.zeros((n, 8))
                ctx.call("ssdseg_mask_head_fwd_dice", logits, n, h, w, 4, 4, 4, y, c4(CW), squared, prob, loss, coef)
                ctx.call("ssdseg_mask_head_fwd_dice", logits, n, h, w, 4, 4, 4, y, c4(CW), squared, None, loss2, coef2)
                return {"prob": prob.download(), "loss": loss.download(), "coef": coef.download(), "loss_without_prob": loss2.download(),
                        "coef_without_prob": coef2.download()}

            for env in ({}, GATHER_MASK):
                @case(f"mask_head_bwd_dice {tag}" + (" gather" if env else ""), env)
                def _(ctx, n=n, h=h, w=w, squared=squared, inputs=inputs):
                    logits, y = inputs(ctx)
                    coef, g = ctx.zeros((n, 8)), ctx.zeros((n, h, w, 4))
                    ctx.call("ssdseg_mask_head_fwd_dice", logits, n, h, w, 4, 4, 4, y, c4(CW), squared, None, None, coef)
                    ctx.call("ssdseg_mask_head_bwd_dice", logits, n, h, w, 4, 4, 4, y, coef, squared, 0.5, g)
                    return {"dlogits": g.download()}


def add_tail_cases():
    @case("head_gather b2 6x8x24 c24 forward with a view, reverse")
    def _(ctx):
        b, elems, c, off, total = 2, 6 * 8 * 24, 24, 28, 6 * 8 * 24 + 40
        x = ctx.array(hashed((b, elems), 15, -4.0, 4.0))
        out = ctx.zeros((b, total))
        ctx.call("ssdseg_head_gather", affine_view(ctx, x, c, 40), out, b, elems, c, off, total, 0)
        back = ctx.zeros((b, elems))
        ctx.call("ssdseg_head_gather", plain_view(out), back, b, elems, c, off, total, 1)
        return {"out": out.download(), "back": back.download()}

    @case("softmax_rows 1000 rows with a view")
    def _(ctx):
        x = ctx.array(hashed((1000, 4), 16, -4.0, 4.0))
        out = ctx.zeros((1000, 4))
        ctx.call("ssdseg_softmax_rows", affine_view(ctx, x, 4, 50), out, 1000, 4)
        return {"out": out.download()}

    @case("metric_mask_iou from logits n2 h12 w16 x4x4")
    def _(ctx):
        n, h, w, f = 2, 12, 16, 4
        out = ctx.zeros((n,))
        ctx.call("ssdseg_metric_mask_iou", ctx.array(hashed((n, h, w, 4), 17, -4.0, 4.0)), n, h, w, 4, f, f, 1,
                 ctx.array(one_hot((n, h * f, w * f), 18)), c4(CW), out)
        return {"out": out.download()}

    @case("metric_mask_iou from probabilities n2 h48 w64")
    def _(ctx):
        n, h, w = 2, 48, 64
        out = ctx.zeros((n,))
        ctx.call("ssdseg_metric_mask_iou", ctx.array(probabilities((n, h, w), 19)), n, h, w, 4, 1, 1, 0, ctx.array(one_hot((n, h, w), 20)), c4(CW), out)
        return {"out": out.download()}

    @case("metric_label_accuracy b3 a600")
    def _(ctx):
        b, a = 3, 600
        p = probabilities((b, a), 21)
        p[0, :3] = 0.25                                       # exact ties: the first class
        out = ctx.zeros((b,))
        ctx.call("ssdseg_metric_label_accuracy", ctx.array(one_hot((b, a), 22)), ctx.array(p), b, a, 4, c4((0.0, 1 / 3, 1 / 3, 1 / 3)), out)
        return {"out": out.download()}

    @case("metric_box_iou b3 a600, image 1 without objects")
    def _(ctx):
        b, a = 3, 600
        positive = (hash32(b * a, 23) >> np.uint64(16)) % np.uint64(16) == 0
        t = hashed((b, a, 4), 24, -2.0, 2.0) * positive.reshape(b, a, 1).astype(np.float32)
        t[1] = 0.0                                            # no objects: 0 / 0, pinned as the bytes of that NaN
        p = hashed((b, a, 4), 25, 0.0, 6.0)
        p[0, : a // 2] = t[0, : a // 2]                       # some perfect predictions
        anchors = np.concatenate([hashed((a, 1), 26, 0.0, 640.0), hashed((a, 1), 27, 0.0, 480.0), hashed((a, 2), 28, 20.0, 300.0)], axis=1)
        out = ctx.zeros((b,))
        ctx.call("ssdseg_metric_box_iou", ctx.array(t), ctx.array(p), ctx.array(anchors), c4(STDS), b, a, out)
        return {"out": out.download()}


add_gap_cases()
add_bilinear_cases()
add_mask_cases()
add_dice_cases()
add_tail_cases()
assert len({name for name, _, _ in CASES}) == len(CASES)

SWITCHES = ("SSDSEG_BILINEAR", "SSDSEG_MASK_BWD")


def observe(ctx, env, fn):
    """the case's calls under its switches, timing registry on -> ({kernel symbol: launches}, {output name: SHA-256 of its bytes})"""
    before = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        outputs = fn(ctx)
        ctx.join()
        launches = {name: r["count"] for name, r in ctx.timing_report().items()}
    finally:
        ctx.timing(False)
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return launches, {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in outputs.items()}


def record(out):
    """prints the table of this build (for EXPECTED: run it on the commit the table is to be taken from, see the module docstring)"""
    from ssdseglib import _hip as H
    ctx = H.Context(0)
    out.write("EXPECTED = {\n")
    for name, env, fn in CASES:
        launches, digests = observe(ctx, env, fn)
        out.write(f"    {name!r}: (\n        {launches!r},\n        {{" + ",\n         ".join(f"{k!r}: {v!r}" for k, v in digests.items()) + "}),\n")
    out.write("}\n")
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("name", [name for name, _, _ in CASES])
def test_heads_launches_and_bits_are_pinned(ctx, name):
    env, fn = next((e, f) for n, e, f in CASES if n == name)
    launches, digests = observe(ctx, env, fn)
    want_launches, want_digests = EXPECTED[name]
    assert launches == want_launches, name
    assert digests == want_digests, (name, [k for k in digests if digests[k] != want_digests.get(k)])


# every kernel of csrc/resize.hip, csrc/mask_head.hip and csrc/heads.hip, under the name its launch leaves in the timing registry
KERNELS = ("gap_fwd_kernel", "chunk_sum_kernel", "gap_bwd_kernel", "bilinear_fwd_kernel", "bilinear_fwd_x4_kernel", "bilinear_bwd_kernel",
           "bilinear_bwd_x4_kernel", "mask_head_fwd_kernel", "mask_loss_final_kernel", "mask_head_fwd_dice_kernel", "mask_dice_final_kernel",
           "mask_head_bwd_kernel", "(mask_head_bwd_tile_kernel<F, TL>)", "(mask_head_bwd_tile_split_kernel<F, TL, PARTS>)",
           "mask_iou_partial_kernel<true>", "mask_iou_partial_kernel<false>", "mask_iou_finish_kernel", "head_gather_kernel",
           "softmax_rows4_kernel", "label_accuracy_kernel", "box_iou_kernel")


def test_expected_table_reaches_every_kernel():
    """the recorded table itself: one entry per case, no empty map or digest list, every kernel of the three units in it"""
    assert set(EXPECTED) == {name for name, _, _ in CASES}
    seen = set()
    for launches, digests in EXPECTED.values():
        assert launches and digests and all(len(d) == 64 for d in digests.values())
        seen.update(launches)
    assert seen == set(KERNELS), seen ^ set(KERNELS)


# Recorded with `record` above, one process, on an MI355X from a checkout of the commit named here (the parent of the commit that
# introduced this module), under the ROCm version named here.  {case: ({kernel symbol: launches}, {output: SHA-256 of its bytes})}
EXPECTED_FROM = "2e7870a4cd41aecf230c1c16238050ad493dc329"
EXPECTED_ROCM = "7.2.0"
EXPECTED = {
    'gap_fwd n2 hw63 c8 affine+relu6': (
        {'gap_fwd_kernel': 1},
        {'out': '33e463d5b74b002128d80fc046cca343fb33a2006c8f143549f19ed566a1b5f0'}),
    'gap_fwd n3 hw1200 c576 affine+relu6': (
        {'chunk_sum_kernel': 1, 'gap_fwd_kernel': 1},
        {'out': '2b3050e44f050498349e68bb36fec13b0318f003cefcb02e240e6a4598d8e822'}),
    'gap_fwd n3 hw1200 c576 identity': (
        {'chunk_sum_kernel': 1, 'gap_fwd_kernel': 1},
        {'out': 'd2564331c86f83b821208c396ce5ec07285e31ab6d2398a7467e463eaebcff1e'}),
    'gap_bwd n3 hw1200 c16 acc0': (
        {'gap_bwd_kernel': 1},
        {'dx': 'aac190fc512546b95d6bce2048ba8ca580fa93ee4b60e84b3469db79ebee804d'}),
    'gap_bwd n3 hw1200 c16 acc1': (
        {'gap_bwd_kernel': 1},
        {'dx': '7394622bd812ece03c4cbc46fd9fb9124dd7e0aac3ea7aa89869bf888093994f'}),
    'bilinear n2 h6 w8 c16 x4x4': (
        {'bilinear_bwd_x4_kernel': 1, 'bilinear_fwd_x4_kernel': 1},
        {'out': '1efa380a1db1b03a47dad6a75adc730d953fd3628f3822a009282bdf42e81093',
         'dx': '799594140e0cdad01ff1abfb425519c314f205890b63d0f31dea37cf262590ed'}),
    'bilinear n2 h6 w8 c16 x4x4 gather': (
        {'bilinear_bwd_kernel': 1, 'bilinear_fwd_kernel': 1},
        {'out': '1efa380a1db1b03a47dad6a75adc730d953fd3628f3822a009282bdf42e81093',
         'dx': '799594140e0cdad01ff1abfb425519c314f205890b63d0f31dea37cf262590ed'}),
    'bilinear n2 h5 w7 c8 x4x4': (
        {'bilinear_bwd_x4_kernel': 1, 'bilinear_fwd_x4_kernel': 1},
        {'out': 'fec2a0f876f800920c75b0cab7911d802103d0959df666a9ad7b2866c60e9ddf',
         'dx': '7137a1769245ce0bc193c7c5fc09d038f038d0fc4951200470143e0357badccd'}),
    'bilinear n2 h5 w7 c8 x4x4 gather': (
        {'bilinear_bwd_kernel': 1, 'bilinear_fwd_kernel': 1},
        {'out': 'fec2a0f876f800920c75b0cab7911d802103d0959df666a9ad7b2866c60e9ddf',
         'dx': '7137a1769245ce0bc193c7c5fc09d038f038d0fc4951200470143e0357badccd'}),
    'bilinear n3 h2 w1 c72 x4x4': (
        {'bilinear_bwd_x4_kernel': 1, 'bilinear_fwd_x4_kernel': 1},
        {'out': 'f075159d22223f4f80b116c36e2c3a924b0403742cee6f4bf1a48efbbe81209e',
         'dx': '843dd8296a98d880d6e9345d8b9a53b0fda5a6016cf5f8745fc166a902671d31'}),
    'bilinear n3 h2 w1 c72 x4x4 gather': (
        {'bilinear_bwd_kernel': 1, 'bilinear_fwd_kernel': 1},
        {'out': 'f075159d22223f4f80b116c36e2c3a924b0403742cee6f4bf1a48efbbe81209e',
         'dx': '843dd8296a98d880d6e9345d8b9a53b0fda5a6016cf5f8745fc166a902671d31'}),
    'bilinear n1 h5 w7 c8 x2x8': (
        {'bilinear_bwd_kernel': 1, 'bilinear_fwd_kernel': 1},
        {'out': '35fd11cad69748beaf21849ffa2e6ef2cb7fc8e653d7809d377c4df437f5bdda',
         'dx': 'ac84c18871dc8b525b3794c12d817b38fe816402c100da1dbeac44b4b8e92197'}),
    'bilinear n1 h3 w3 c4 x1x1': (
        {'bilinear_bwd_kernel': 1, 'bilinear_fwd_kernel': 1},
        {'out': '3114ae152185474da200fe8e2bcba3759009c75d3f83d5a6f0c5eed25073e6db',
         'dx': 'f3f98738399b7289b2bcfde59f1c69df6cd639448e8c113980514096f72d0580'}),
    'bilinear_bwd pixel sum n2 c256 x30x40 acc0': (
        {'chunk_sum_kernel': 1, 'gap_fwd_kernel': 1},
        {'dx': '9365647b37dda95f3d245682fb6db0a0d242d3e6aec5f275db6fcf9faccccf00'}),
    'bilinear_bwd pixel sum n2 c256 x30x40 acc1': (
        {'chunk_sum_kernel': 1, 'gap_fwd_kernel': 1},
        {'dx': 'a3ea33a206e826a8f36ffc1b5f0afb0724cf9e836479e4064741152351c1875c'}),
    'bilinear wide rows and padded n2 h5 w7 c8 x4x4': (
        {'bilinear_bwd_x4_kernel': 1, 'bilinear_fwd_x4_kernel': 2},
        {'out': '8911ada3546ad38d38e89e6bf1a26dd3f12d315711fe7cc744481687853b5dbc',
         'padded': '0fd1c8b7fb930be6c624c5a6b39bd07bca5839e2a627bf79b87b3e13d2b3f896',
         'dx': 'c702912f31ee8a6717c14c019ec85320a8866a5054a4f4710a8fbffcdbd0cbe1'}),
    'bilinear wide rows and padded n2 h5 w7 c8 x4x4 gather': (
        {'bilinear_bwd_kernel': 1, 'bilinear_fwd_kernel': 2},
        {'out': '8911ada3546ad38d38e89e6bf1a26dd3f12d315711fe7cc744481687853b5dbc',
         'padded': '0fd1c8b7fb930be6c624c5a6b39bd07bca5839e2a627bf79b87b3e13d2b3f896',
         'dx': 'c702912f31ee8a6717c14c019ec85320a8866a5054a4f4710a8fbffcdbd0cbe1'}),
    'mask_head_fwd n2 h12 w16 x4x4': (
        {'mask_head_fwd_kernel': 3, 'mask_loss_final_kernel': 2},
        {'prob': '42ed43bb605e23b7af062b56e19dbdaf8b815008f01b69dc39087bf61208024c',
         'loss': '39602f3a6f558c30825d8093d164051a7200a43a845f5f0634382089a7a7c8ae',
         'prob_only': '42ed43bb605e23b7af062b56e19dbdaf8b815008f01b69dc39087bf61208024c',
         'loss_only': '39602f3a6f558c30825d8093d164051a7200a43a845f5f0634382089a7a7c8ae'}),
    'mask_head_bwd n2 h12 w16 x4x4': (
        {'(mask_head_bwd_tile_kernel<F, TL>)': 1},
        {'dlogits': 'bf7ce727acde8d7b2c86deeb7537745f9c6ccc9e477b3608b75873849dc0a1bd'}),
    'mask_head_bwd n2 h12 w16 x4x4 gather': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': 'bf7ce727acde8d7b2c86deeb7537745f9c6ccc9e477b3608b75873849dc0a1bd'}),
    'mask_head_fwd n1 h17 w35 x4x4': (
        {'mask_head_fwd_kernel': 3, 'mask_loss_final_kernel': 2},
        {'prob': 'cc9a2501c44dfee8038595e61d4e316e5dc5f0648fa85ccbf4bfc14dac35bbcc',
         'loss': 'd6e3f89cee0586694eb04cc309e44ebb8ff60f8199b1b25fc5421e2ccf0b7869',
         'prob_only': 'cc9a2501c44dfee8038595e61d4e316e5dc5f0648fa85ccbf4bfc14dac35bbcc',
         'loss_only': 'd6e3f89cee0586694eb04cc309e44ebb8ff60f8199b1b25fc5421e2ccf0b7869'}),
    'mask_head_bwd n1 h17 w35 x4x4': (
        {'(mask_head_bwd_tile_kernel<F, TL>)': 1},
        {'dlogits': '1581ce82942026c14b4bb9877d43899442bc27e4772c7799daa9765513bf02b1'}),
    'mask_head_bwd n1 h17 w35 x4x4 gather': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': '1581ce82942026c14b4bb9877d43899442bc27e4772c7799daa9765513bf02b1'}),
    'mask_head_fwd n3 h5 w3 x4x4': (
        {'mask_head_fwd_kernel': 3, 'mask_loss_final_kernel': 2},
        {'prob': '81d2276e48b29d80ebff67e6ede1ffd429bfaffb247eb9ccacf169d7b418bbad',
         'loss': '670c59e0143a9d83924a2ed7507bf53f4ad1f261014e2c5dcd008919e9938751',
         'prob_only': '81d2276e48b29d80ebff67e6ede1ffd429bfaffb247eb9ccacf169d7b418bbad',
         'loss_only': '670c59e0143a9d83924a2ed7507bf53f4ad1f261014e2c5dcd008919e9938751'}),
    'mask_head_bwd n3 h5 w3 x4x4': (
        {'(mask_head_bwd_tile_kernel<F, TL>)': 1},
        {'dlogits': '3b59fe14f1fe102fa28d182e858b1267a90ff4b0573b5b22066ac6ea3680b5e7'}),
    'mask_head_bwd n3 h5 w3 x4x4 gather': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': '3b59fe14f1fe102fa28d182e858b1267a90ff4b0573b5b22066ac6ea3680b5e7'}),
    'mask_head_fwd n2 h12 w16 x8x8': (
        {'mask_head_fwd_kernel': 3, 'mask_loss_final_kernel': 2},
        {'prob': 'b82b7a21e9bc680f8b409279e4908c4c51aed7fde0b113611b19db294db91c1e',
         'loss': '53aa9aafc4df79903b30cbf67d4417e80600f56cc44854785ea8bc9f6a84e194',
         'prob_only': 'b82b7a21e9bc680f8b409279e4908c4c51aed7fde0b113611b19db294db91c1e',
         'loss_only': '53aa9aafc4df79903b30cbf67d4417e80600f56cc44854785ea8bc9f6a84e194'}),
    'mask_head_bwd n2 h12 w16 x8x8': (
        {'(mask_head_bwd_tile_split_kernel<F, TL, PARTS>)': 1},
        {'dlogits': '69f87c1d7bb57840284349a2d078b8d77bf12c223a5c904fe2ccab98c8f2a981'}),
    'mask_head_bwd n2 h12 w16 x8x8 gather': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': '30250a42535ea30a468a7f1ab94f538cbf435e8508241c8ff4c50946d8fb9153'}),
    'mask_head_fwd n1 h17 w35 x8x8': (
        {'mask_head_fwd_kernel': 3, 'mask_loss_final_kernel': 2},
        {'prob': '27e2dcf94e0866e3abc4acb6950f4e38144a97a1689e93769ddbcfa5a33ab3fc',
         'loss': '7846ab5552887c0b861414ff3afedd0217a4cdcc08c2cbd56197d50ade16da85',
         'prob_only': '27e2dcf94e0866e3abc4acb6950f4e38144a97a1689e93769ddbcfa5a33ab3fc',
         'loss_only': '7846ab5552887c0b861414ff3afedd0217a4cdcc08c2cbd56197d50ade16da85'}),
    'mask_head_bwd n1 h17 w35 x8x8': (
        {'(mask_head_bwd_tile_split_kernel<F, TL, PARTS>)': 1},
        {'dlogits': 'b8aa4ba64bc31dc7589b1766a0130e0f42e7bfec6141c0064ca42811de81675b'}),
    'mask_head_bwd n1 h17 w35 x8x8 gather': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': 'f69be34aff1cdb7eeafa181e23e4f540465a7abe95c9a00324c887a0d39ee6f9'}),
    'mask_head_fwd n3 h5 w3 x8x8': (
        {'mask_head_fwd_kernel': 3, 'mask_loss_final_kernel': 2},
        {'prob': '95f1f0b57fd185bd5153d46da3ece3b62fe54b8bf80ad1f4333677e5cc0c7857',
         'loss': 'f08c9e2c64dc47d126351e7d17fb96110f589d0630bdf6214a13915185701934',
         'prob_only': '95f1f0b57fd185bd5153d46da3ece3b62fe54b8bf80ad1f4333677e5cc0c7857',
         'loss_only': 'f08c9e2c64dc47d126351e7d17fb96110f589d0630bdf6214a13915185701934'}),
    'mask_head_bwd n3 h5 w3 x8x8': (
        {'(mask_head_bwd_tile_split_kernel<F, TL, PARTS>)': 1},
        {'dlogits': '7f0408f53113ae91311490ab77bbaecca6d620e957236f896f3da182e9a2ed4e'}),
    'mask_head_bwd n3 h5 w3 x8x8 gather': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': 'f21cf2de0391198555accda3ff97a1293032693e2a633fa99cb20f78b92c23cc'}),
    'mask_head_fwd n1 h5 w7 x2x8': (
        {'mask_head_fwd_kernel': 3, 'mask_loss_final_kernel': 2},
        {'prob': '6da49a4f68e8a582dfe45607cbe51768e5ce7809ef77d9d0dc01bac5dce0feff',
         'loss': 'd747ea1c6aa778514e0ff7ab51f0330261da1f3cd9f9bb85567ca60e5a271794',
         'prob_only': '6da49a4f68e8a582dfe45607cbe51768e5ce7809ef77d9d0dc01bac5dce0feff',
         'loss_only': 'd747ea1c6aa778514e0ff7ab51f0330261da1f3cd9f9bb85567ca60e5a271794'}),
    'mask_head_bwd n1 h5 w7 x2x8': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': 'd5b047477800183ebc48c079cb71a25cb73ca2ffcb96466ea086b778f0b8bb42'}),
    'mask_head_bwd n1 h5 w7 x2x8 gather': (
        {'mask_head_bwd_kernel': 1},
        {'dlogits': 'd5b047477800183ebc48c079cb71a25cb73ca2ffcb96466ea086b778f0b8bb42'}),
    'mask_head_fwd_dice n2 h6 w8 x4x4 squared0': (
        {'mask_dice_final_kernel': 2, 'mask_head_fwd_dice_kernel': 2},
        {'prob': '760c3cb07ef0900303bfdcc510422a63eba2199e3d37bf00d4a97668cd447d44',
         'loss': 'b211ed729d5252843368b21802b8fa5ce5cef4a366fe7436e2b5d7af2db6175f',
         'coef': '6275febe84fc56091150817095132aeac42f962f759ce264a3c0d5a52ed8e178',
         'loss_without_prob': 'b211ed729d5252843368b21802b8fa5ce5cef4a366fe7436e2b5d7af2db6175f',
         'coef_without_prob': '6275febe84fc56091150817095132aeac42f962f759ce264a3c0d5a52ed8e178'}),
    'mask_head_bwd_dice n2 h6 w8 x4x4 squared0': (
        {'(mask_head_bwd_tile_kernel<F, TL>)': 1, 'mask_dice_final_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': 'b0fba9434fcce759ed83cf11bfd295bcdfa509c2ab6bad9e6a498a623c8985ae'}),
    'mask_head_bwd_dice n2 h6 w8 x4x4 squared0 gather': (
        {'mask_dice_final_kernel': 1, 'mask_head_bwd_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': 'b0fba9434fcce759ed83cf11bfd295bcdfa509c2ab6bad9e6a498a623c8985ae'}),
    'mask_head_fwd_dice n2 h6 w8 x4x4 squared1': (
        {'mask_dice_final_kernel': 2, 'mask_head_fwd_dice_kernel': 2},
        {'prob': '760c3cb07ef0900303bfdcc510422a63eba2199e3d37bf00d4a97668cd447d44',
         'loss': 'a704b93ffb82a11635f9dfd11593baeb5fa0cbd2a05991096637fba6a651891d',
         'coef': '97bae206e54e6259559e16770e966b85e76999afed9a4cb7f078c7d376377be0',
         'loss_without_prob': 'a704b93ffb82a11635f9dfd11593baeb5fa0cbd2a05991096637fba6a651891d',
         'coef_without_prob': '97bae206e54e6259559e16770e966b85e76999afed9a4cb7f078c7d376377be0'}),
    'mask_head_bwd_dice n2 h6 w8 x4x4 squared1': (
        {'(mask_head_bwd_tile_kernel<F, TL>)': 1, 'mask_dice_final_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': '24c230a56a49c64f6a89272c0c6324da91f04a8ddf1ea25df5d04a129cb2be4d'}),
    'mask_head_bwd_dice n2 h6 w8 x4x4 squared1 gather': (
        {'mask_dice_final_kernel': 1, 'mask_head_bwd_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': '24c230a56a49c64f6a89272c0c6324da91f04a8ddf1ea25df5d04a129cb2be4d'}),
    'mask_head_fwd_dice n3 h30 w40 x4x4 squared0': (
        {'mask_dice_final_kernel': 2, 'mask_head_fwd_dice_kernel': 2},
        {'prob': '5f49e7762ebeebf78403674e14fcea8f04f563e29f31e2dc9c5ec2e5c2e42b72',
         'loss': 'd382d7fced4321b83c0492d6c489e93cab4703c93d4b3f37e9d97825da5ed55c',
         'coef': '1cdd988f46ed9a3d5fa6b9e9d36b11b8d2df7f4f462f49473725a327677a3907',
         'loss_without_prob': 'd382d7fced4321b83c0492d6c489e93cab4703c93d4b3f37e9d97825da5ed55c',
         'coef_without_prob': '1cdd988f46ed9a3d5fa6b9e9d36b11b8d2df7f4f462f49473725a327677a3907'}),
    'mask_head_bwd_dice n3 h30 w40 x4x4 squared0': (
        {'(mask_head_bwd_tile_kernel<F, TL>)': 1, 'mask_dice_final_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': '8febc973c451fa448bf892d538cdbbc9999b9862e5aa965dbe65296e0a3c1ab3'}),
    'mask_head_bwd_dice n3 h30 w40 x4x4 squared0 gather': (
        {'mask_dice_final_kernel': 1, 'mask_head_bwd_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': '8febc973c451fa448bf892d538cdbbc9999b9862e5aa965dbe65296e0a3c1ab3'}),
    'mask_head_fwd_dice n3 h30 w40 x4x4 squared1': (
        {'mask_dice_final_kernel': 2, 'mask_head_fwd_dice_kernel': 2},
        {'prob': '5f49e7762ebeebf78403674e14fcea8f04f563e29f31e2dc9c5ec2e5c2e42b72',
         'loss': '36908fc4b6482b7f643822eb4b86fb692b5fd8be1c99e447287e80e4a06a0646',
         'coef': 'c149eac855e7269dbcd541e72e217f6ba91bb3fb20a84bd767651f1cc803f1dc',
         'loss_without_prob': '36908fc4b6482b7f643822eb4b86fb692b5fd8be1c99e447287e80e4a06a0646',
         'coef_without_prob': 'c149eac855e7269dbcd541e72e217f6ba91bb3fb20a84bd767651f1cc803f1dc'}),
    'mask_head_bwd_dice n3 h30 w40 x4x4 squared1': (
        {'(mask_head_bwd_tile_kernel<F, TL>)': 1, 'mask_dice_final_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': 'e339989b03b0686a76421ad750b8b2ad245f612bd55a0365693cc56ae773cd92'}),
    'mask_head_bwd_dice n3 h30 w40 x4x4 squared1 gather': (
        {'mask_dice_final_kernel': 1, 'mask_head_bwd_kernel': 1, 'mask_head_fwd_dice_kernel': 1},
        {'dlogits': 'e339989b03b0686a76421ad750b8b2ad245f612bd55a0365693cc56ae773cd92'}),
    'head_gather b2 6x8x24 c24 forward with a view, reverse': (
        {'head_gather_kernel': 2},
        {'out': '2ffa2cb319b1d732fdbf2e5fc9589f0be156220fdcc36fabfbebe43fe18092c1',
         'back': 'df7c5884a615e5e6555c2c2e60111b90b1625e06ad1fcaae31927839b8f93b1e'}),
    'softmax_rows 1000 rows with a view': (
        {'softmax_rows4_kernel': 1},
        {'out': '818f610eb8c41688f427542b4f80b6c1e3fc8918d75d986b86b85bfd79041799'}),
    'metric_mask_iou from logits n2 h12 w16 x4x4': (
        {'mask_iou_finish_kernel': 1, 'mask_iou_partial_kernel<true>': 1},
        {'out': '11178ea7374d38965eb1815350f17bb7e44810a5472b9b4b7cfcccb6cd613dcd'}),
    'metric_mask_iou from probabilities n2 h48 w64': (
        {'mask_iou_finish_kernel': 1, 'mask_iou_partial_kernel<false>': 1},
        {'out': 'b585e0209b9002f234914e57f0f287c31bd26babd1425879670c1a1af38106af'}),
    'metric_label_accuracy b3 a600': (
        {'label_accuracy_kernel': 1},
        {'out': '91094a65426ce7b0cda01513101158e80af1714ed9091532e2ef358895561810'}),
    'metric_box_iou b3 a600, image 1 without objects': (
        {'box_iou_kernel': 1},
        {'out': '04156a78a272cd57bb12f13abfed9b780a05b636fdfe47e865bf782edaec6c97'}),
}
