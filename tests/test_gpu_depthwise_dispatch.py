"""GPU: which kernels the depthwise-conv entry points launch, per shape, operand form and kernel family -- pinned.

The host half of csrc/dwconv.hip turns (shape, stride, dilation, operand form, switches) into a plan: a kernel family, one
instantiation of that family's kernel template, a grid and a partial-table size.  The parity tests see a wrong choice only when it
is also a wrong result; this module sees it as such: every case makes ONE call with the timing registry on and compares the
{kernel symbol: launches} map it leaves with the map recorded from the parent of the commit that introduced this test
(EXPECTED_FROM, by running `observe` below on a checkout of it) -- never from the code under test.  No uploads and no oracle: the
buffers stay as allocated, the values do not matter.

The shapes reach both values of every template flag: widths that are and are not a multiple of the 4-column strip (WFULL), the
four stride-2 pad pairs (PT, PL), one, two and several channel chunks, c > 160 (the register-window backward when the marches are
off) and two dilations (DIL; D2 is the forward's two-rows-ahead form, off in two families); the forms reach BNFUSE and ACC.  On
top of the families of tests/conftest.py, SSDSEG_DW_ATROUS=gather, SSDSEG_DW_BWD=march and SSDSEG_DW_FWD_DEPTH=1 are set, one at a
time, over the default family.

The one path no small test can reach: tensors of >= 2^30 elements, which the marching kernels (32-bit byte offsets) leave to the
LDS-tiled, register-window and gather kernels.
"""
import itertools

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [
    # n, h, w, c, stride, dilation
    (1, 8, 12, 32, 1, 1),      # w % 4 == 0
    (1, 8, 10, 32, 1, 1),
    (1, 9, 7, 8, 2, 1), (1, 10, 7, 8, 2, 1), (1, 9, 8, 8, 2, 1), (1, 10, 8, 8, 2, 1),      # pads (1,1) (0,1) (1,0) (0,0)
    (1, 12, 16, 128, 1, 1),    # two 64-channel chunks
    (1, 6, 8, 144, 1, 1),      # one 144-channel chunk
    (1, 5, 6, 1284, 1, 1),     # six chunks; 321 channel vectors
    (1, 9, 10, 192, 1, 1),     # c > 160
    (2, 7, 5, 8, 1, 3),        # atrous, ragged sub-grids
    (1, 4, 5, 8, 1, 12),       # dilation > image
]

# entry point : operand form
FORMS = ["fwd:stats", "fwd:plain"] + \
        [f"bwd:{gv}+{dx}+acc{a}" for gv, dx, a in itertools.product(("identity", "bn"), ("dx", "nodx"), (0, 1))] + \
        ["bwd_bn:acc0", "bwd_bn:acc1"]

FAMILIES = ["default", "general", "general-reg", "resident-fused", "tile", "tile-32", "tile-wide"]
# switches set on top of the default family, recorded under these names next to the families
SWITCHES = {"atrous=gather": ("SSDSEG_DW_ATROUS", "gather"), "bwd=march": ("SSDSEG_DW_BWD", "march"),
            "fwd_depth=1": ("SSDSEG_DW_FWD_DEPTH", "1")}      # (the last: the one-row-ahead forward march, which no family runs)
DW_VARS = ("SSDSEG_DW_FWD", "SSDSEG_DW_BWD", "SSDSEG_DW_FWD_DEPTH", "SSDSEG_DW_ATROUS")

ACT_RELU6 = 2
STATS_ROWS = 256       # (ssdseg_dwconv_parts asks for at most 144 rows at these shapes)


class Pool:
    """device buffers large enough for every shape, allocated once and never written by the host"""

    def __init__(self, ctx):
        elems = max(n * h * w * c for n, h, w, c, s, d in SHAPES)
        cmax = max(c for n, h, w, c, s, d in SHAPES)
        self.x, self.dx, self.y, self.g, self.yraw = (ctx.empty((elems,)) for _ in range(5))
        self.w, self.dw = ctx.empty((9 * cmax,)), ctx.empty((9 * cmax,))
        self.vec = [ctx.empty((cmax,)) for _ in range(12)]
        self.stats = ctx.empty((STATS_ROWS * 2 * cmax,))


def observe(ctx, pool, form, n, h, w, c, s, d):
    """one call of the entry point in the given operand form -> {kernel symbol: launches}"""
    from ssdseglib import _hip as H
    entry, _, what = form.partition(":")
    what = what.split("+")
    v = pool.vec
    ho, wo = -(-h // s), -(-w // s)
    xin = H.view(pool.x.view(0, (n, h, w, c)), v[0].view(0, (c,)), v[1].view(0, (c,)), ACT_RELU6)
    g, yraw = pool.g.view(0, (n, ho, wo, c)), pool.yraw.view(0, (n, ho, wo, c))
    gv = H.gview(g) if "identity" in what else H.gview(g, yraw, *(b.view(0, (c,)) for b in v[2:6]), act=ACT_RELU6)
    wgt, dw, dx = pool.w.view(0, (3, 3, c)), pool.dw.view(0, (3, 3, c)), pool.dx.view(0, (n, h, w, c))
    acc = 1 if "acc1" in what else 0
    ctx.timing(True)
    ctx.timing_reset()
    try:
        if entry == "fwd":
            nparts = ctx.parts("ssdseg_dwconv_parts", n, h, w, c, s, d)
            assert nparts <= STATS_ROWS
            stats = pool.stats.view(0, (nparts, 2, c)) if "stats" in what else None
            ctx.call("ssdseg_dwconv_fwd", xin, wgt, pool.y.view(0, (n, ho, wo, c)), n, h, w, c, s, d, stats)
        elif entry == "bwd":
            ctx.call("ssdseg_dwconv_bwd", xin, wgt, gv, None if "nodx" in what else dx, dw, n, h, w, c, s, d, acc)
        elif entry == "bwd_bn":
            outs = [b.view(0, (c,)) for b in v[8:12]]
            ctx.call("ssdseg_dwconv_bwd_bn", xin, wgt, gv, dx, dw, n, h, w, c, s, d, acc, v[6].view(0, (c,)), v[7].view(0, (c,)), *outs)
        else:
            raise ValueError(form)
        ctx.join()
        return {name: r["count"] for name, r in ctx.timing_report().items()}
    finally:
        ctx.timing(False)


@pytest.fixture(scope="module")
def pool(ctx):
    return Pool(ctx)


def expected(form, shape, setting):
    for settings, want in EXPECTED[(form,) + shape].items():
        if setting in settings.split():
            return want
    raise KeyError((form, shape, setting))


def check(ctx, pool, shape, setting):
    for form in FORMS:
        got = observe(ctx, pool, form, *shape)
        want = expected(form, shape, setting)
        assert want, (form, shape, setting)
        assert got == want, (form, shape, setting)


@pytest.mark.parametrize("shape", SHAPES)
def test_depthwise_dispatch_is_pinned(ctx, pool, kernel_family, shape):
    check(ctx, pool, shape, kernel_family)


@pytest.mark.parametrize("setting", list(SWITCHES))
def test_depthwise_dispatch_under_a_switch_is_pinned(ctx, pool, monkeypatch, setting):
    for k in DW_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(*SWITCHES[setting])
    for shape in SHAPES:
        check(ctx, pool, shape, setting)


def test_expected_table_reaches_every_branch():
    """the recorded table itself: no empty map, and every kernel template and every value of every template flag appears in it"""
    seen = set()
    for per_setting in EXPECTED.values():
        assert sorted(f for fams in per_setting for f in fams.split()) == sorted(FAMILIES + list(SWITCHES))
        for want in per_setting.values():
            assert want
            seen.update(want)
    assert set(EXPECTED) == {(form,) + shape for form in FORMS for shape in SHAPES}

    def args(template):
        """the argument tuples of the recorded instantiations of one kernel template"""
        found = [s[len(template) + 2:-2].split(", ") for s in seen if s.startswith(f"({template}<")]
        assert found, template
        return found

    def both(template, position, values=("true", "false")):
        have = {a[position] for a in args(template) if len(a) > position}
        assert have >= set(values), (template, position, have)

    for flag in range(4):                                      # BNFUSE, WFULL, ACC, DIL
        both("dw_bwd_march_kernel", flag)
    both("dw_bwd_march2_kernel", 0)                            # BNFUSE
    both("dw_bwd_march2_kernel", 3)                            # ACC
    for template, first in (("dw_bwd_march2_kernel", 1), ("dw_fwd_march_kernel", 1), ("dw_bwd_kernel", 2)):
        both(template, first, "01")                            # PT
        both(template, first + 1, "01")                        # PL
    both("dw_fwd_march_kernel", 0, "12")                       # S
    both("dw_fwd_march_kernel", 3)                             # DIL
    assert any(len(a) == 5 and a[4] == "true" for a in args("dw_fwd_march_kernel"))       # D2 (false: the default, not spelled)
    assert any(len(a) == 4 for a in args("dw_fwd_march_kernel"))
    both("dw_bwd_kernel", 0, "12")                             # S
    both("dw_bwd_kernel", 1, "01")                             # dense taps | gather
    assert args("dw_bwd_lds_kernel") == [["1", "1", "1"]]
    both("dw_fwd_lds_kernel", 0, "12")
    assert args("dw_fwd_kernel") == [["1", "0"]]
    assert "bn_bwd_finalize_kernel" in seen and "colsum_kernel" in seen


# Recorded at the commit named here with `observe` above, one process, every family of tests/conftest.py and the three switches in turn.
# {(form, n, h, w, c, stride, dilation): {"settings that share a map": {kernel symbol: launches}}}
EXPECTED_FROM = "9d7ab19a2672a42359f91174fe1b9078f7d32e6a"
EXPECTED = {
    ('fwd:stats', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('fwd:plain', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('bwd:identity+dx+acc0', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, true, false, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 8, 12, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, true, true, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('fwd:plain', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('bwd:identity+dx+acc0', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, false, false, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 8, 10, 32, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, false, true, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 1, 1, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('fwd:plain', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 1, 1, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('bwd:identity+dx+acc0', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 1, 1, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 9, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 1, 1, true>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 0, 1, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('fwd:plain', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 0, 1, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('bwd:identity+dx+acc0', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 1, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 0, 1, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 10, 7, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 0, 1, true>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 1, 0, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('fwd:plain', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 1, 0, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('bwd:identity+dx+acc0', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 1, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 1, 0, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 9, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 1, 0, true>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 1, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 0, 0, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('fwd:plain', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<2, 0, 0, false>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<2>)": 1}},
    ('bwd:identity+dx+acc0', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, true>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<false, 0, 0, false>)": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 0, 0, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 10, 8, 8, 2, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march2_kernel<true, 0, 0, true>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general general-reg": {"(dw_bwd_kernel<2, 1, 0, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('fwd:plain', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('bwd:identity+dx+acc0', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, true, false, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 12, 16, 128, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, true, true, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('fwd:plain', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('bwd:identity+dx+acc0', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, true, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, true, false, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 6, 8, 144, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, true, true, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('fwd:plain', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('bwd:identity+dx+acc0', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, false, false, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 5, 6, 1284, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, false, true, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('fwd:plain', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march": {"(dw_fwd_march_kernel<1, 1, 1, false, true>)": 1}, "general general-reg": {"(dw_fwd_lds_kernel<1>)": 1}, "fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, false>)": 1}},
    ('bwd:identity+dx+acc0', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, false>)": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, false, false, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 9, 10, 192, 1, 1): {"default resident-fused tile tile-32 tile-wide atrous=gather bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<true, false, true, false>)": 1, "bn_bwd_finalize_kernel": 1, "colsum_kernel": 1}, "general": {"(dw_bwd_lds_kernel<1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general-reg": {"(dw_bwd_kernel<1, 1, 1, 1>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, true>)": 1}, "general general-reg atrous=gather": {"(dw_fwd_kernel<1, 0>)": 1}},
    ('fwd:plain', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, true>)": 1}, "general general-reg atrous=gather": {"(dw_fwd_kernel<1, 0>)": 1}},
    ('bwd:identity+dx+acc0', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 2, 7, 5, 8, 1, 3): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('fwd:stats', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, true>)": 1}, "general general-reg atrous=gather": {"(dw_fwd_kernel<1, 0>)": 1}},
    ('fwd:plain', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_fwd_march_kernel<1, 1, 1, true>)": 1}, "general general-reg atrous=gather": {"(dw_fwd_kernel<1, 0>)": 1}},
    ('bwd:identity+dx+acc0', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+dx+acc1', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc0', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:identity+nodx+acc1', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc0', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+dx+acc1', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc0', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd:bn+nodx+acc1', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc0', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, false, true>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
    ('bwd_bn:acc1', 1, 4, 5, 8, 1, 12): {"default resident-fused tile tile-32 tile-wide bwd=march fwd_depth=1": {"(dw_bwd_march_kernel<false, false, true, true>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}, "general general-reg atrous=gather": {"(dw_bwd_kernel<1, 0, 0, 0>)": 1, "bn_bwd_finalize_kernel": 1, "bn_bwd_partial_kernel": 1, "colsum_kernel": 1}},
}
