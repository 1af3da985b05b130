// Depthwise 3x3 convolution, NHWC fp32, TF SAME padding, stride 1|2, dilation >= 1 (stride 1 only when dilated).
// Replaces DepthwiseConv2D / the depthwise half of SeparableConv2D (reference models.py:88,236,242;
// blocks.py:33,38,43,122,152) forward and backward.
//
// HBM-bound (0.9-2.25 FLOP/B).  Mapping: one thread owns ONE 4-channel vector (16 B) for its whole life, so the
// 9 filter taps, the producer's BN scale/shift and the BN-stat / dW accumulators live in registers; consecutive
// lanes hold consecutive channel vectors, i.e. a wave reads whole contiguous NHWC pixels (C*4 bytes each).
// Each thread walks a grid-strided list of 1x4 output strips and slides a register window along W
// (18 loads per 4 outputs at stride 1 instead of 36); vertical reuse is left to L1/L2.
// BatchNorm(train) is fused on both sides: the producer's normalise+ReLU6 is applied on load (ssdseg_view),
// and this layer's per-channel (sum, sumsq) leave as one partial row per block (no atomics, deterministic).
#include "common.h"

namespace {

constexpr int TW = 4;           // outputs per strip
constexpr int MAX_BLOCKS = 1024;  // also the number of BN-stat / dW partial rows

struct DwGeom {
    int n, h, w, c, ho, wo, s, d, pt, pl;
    int cv;       // c / 4
    int wtiles;   // ceil(wo / TW)
    long long ntiles;
};

struct ViewDev {
    const float* x;
    const float* scale;
    const float* shift;
    int act;
};
struct GViewDev {
    const float* g;
    const float* y;
    const float* scale;
    const float* shift;
    const float* k1;
    const float* k0;
    int act;
};

struct ChanCoef {  // per-thread channel-vector constants (identity views: s = 1, t = k1 = k0 = 0)
    float4 s, t, k1, k0;
    float lo, hi;  // activation clamp of an input view
    bool affine;
};

__device__ __forceinline__ float4 load_view(const ViewDev& v, const ChanCoef& cc, long long off) {
    return view_affine4(ld4(v.x + off), cc.s, cc.t, cc.lo, cc.hi);
}
__device__ __forceinline__ float4 load_gview(const GViewDev& v, const ChanCoef& cc, long long off) {
    return gview_apply4(ld4(v.g + off), ld4(v.y + off), cc.s, cc.t, cc.k1, cc.k0, v.act);
}
// predicated forms: the load is unconditional (address clamped to the thread's own channel vector of pixel 0) and the result
// selected, so the compiler can issue a whole window of loads back to back instead of branch + wait per element
__device__ __forceinline__ float4 sel4(bool ok, float4 v) { return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 load_view_if(const ViewDev& v, const ChanCoef& cc, long long off, bool ok, int c0) {
    return sel4(ok, load_view(v, cc, ok ? off : (long long)c0));
}
__device__ __forceinline__ float4 load_gview_if(const GViewDev& v, const ChanCoef& cc, long long off, bool ok, int c0) {
    return sel4(ok, load_gview(v, cc, ok ? off : (long long)c0));
}
__device__ __forceinline__ void fma4(float4& acc, float4 a, float4 b) {
    acc.x = fmaf(a.x, b.x, acc.x); acc.y = fmaf(a.y, b.y, acc.y); acc.z = fmaf(a.z, b.z, acc.z); acc.w = fmaf(a.w, b.w, acc.w);
}

// block-level reduction over threadIdx.y of one float4 per thread; result valid for threadIdx.y == 0
__device__ __forceinline__ float4 reduce_over_y(float4 v, float4* red) {
    __syncthreads();
    red[threadIdx.y * blockDim.x + threadIdx.x] = v;
    __syncthreads();
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.y == 0) {
        for (int y = 0; y < (int)blockDim.y; ++y) add4(r, red[y * blockDim.x + threadIdx.x]);
    }
    return r;
}

// ------------------------------------------------------------------------------------------------ forward
// S: stride (1|2); DIL: 1 = dense taps with sliding window, 0 = runtime dilation (stride 1), direct gathers.
template <int S, int DIL>
__global__ void __launch_bounds__(512) dw_fwd_kernel(DwGeom gm, ViewDev in, const float* __restrict__ wgt,
                                                     float* __restrict__ y, float* __restrict__ stats) {
    extern __shared__ float4 red[];
    const BlockPos bpos = xcd_block_pos();   // (tile slot, channel group), neighbouring slots on the same XCD / L2
    const int cvi = bpos.y * blockDim.x + threadIdx.x;
    const bool active = cvi < gm.cv;
    const int c0 = cvi * 4;
    float4 wk[9];
    ChanCoef cc;
    cc.affine = in.scale != nullptr;
    cc.s = f4(1.f);
    cc.t = cc.k1 = cc.k0 = f4(0.f);
    cc.lo = act_lo(in.act);
    cc.hi = act_hi(in.act);
    if (active) {
#pragma unroll
        for (int t = 0; t < 9; ++t) wk[t] = ld4(wgt + (long long)t * gm.c + c0);
        if (cc.affine) { cc.s = ld4(in.scale + c0); cc.t = ld4(in.shift + c0); }
    }
    float4 ssum = f4(0.f), ssq = f4(0.f);
    if (active) {
        for (long long tile = (long long)bpos.x * blockDim.y + threadIdx.y; tile < gm.ntiles;
             tile += (long long)gridDim.x * blockDim.y) {
            const int wt = (int)(tile % gm.wtiles);
            const long long r = tile / gm.wtiles;
            const int ho = (int)(r % gm.ho);
            const int n = (int)(r / gm.ho);
            const int wo0 = wt * TW;
            float4 out[TW];
#pragma unroll
            for (int j = 0; j < TW; ++j) out[j] = f4(0.f);
            const long long img = (long long)n * gm.h * gm.w;
            if (DIL == 1) {
                constexpr int WC = (TW - 1) * S + 3;
                const int wi0 = wo0 * S - gm.pl;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int hi = ho * S + kh - gm.pt;
                    const bool rowok = hi >= 0 && hi < gm.h;
                    float4 row[WC];
#pragma unroll
                    for (int ci = 0; ci < WC; ++ci) {
                        const int wi = wi0 + ci;
                        row[ci] = load_view_if(in, cc, ((img + (long long)hi * gm.w + wi) * gm.c) + c0, rowok && wi >= 0 && wi < gm.w, c0);
                    }
#pragma unroll
                    for (int j = 0; j < TW; ++j)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) fma4(out[j], row[j * S + kw], wk[kh * 3 + kw]);
                }
            } else {
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int hi = ho + kh * gm.d - gm.pt;
                    const bool rowok = hi >= 0 && hi < gm.h;
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
                        for (int j = 0; j < TW; ++j) {
                            const int wi = wo0 + j + kw * gm.d - gm.pl;
                            fma4(out[j], load_view_if(in, cc, ((img + (long long)hi * gm.w + wi) * gm.c) + c0,
                                                      rowok && wi >= 0 && wi < gm.w && wo0 + j < gm.wo, c0), wk[kh * 3 + kw]);
                        }
                    }
                }
            }
            const long long obase = (((long long)n * gm.ho + ho) * gm.wo + wo0) * gm.c + c0;
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                if (wo0 + j < gm.wo) {
                    st4(y + obase + (long long)j * gm.c, out[j]);
                    add4(ssum, out[j]);
                    fma4(ssq, out[j], out[j]);
                }
            }
        }
    }
    if (stats != nullptr) {
        float4 a = reduce_over_y(ssum, red);
        float4 b = reduce_over_y(ssq, red);
        if (threadIdx.y == 0 && active) {
            float* row = stats + (long long)bpos.x * 2 * gm.c;
            st4(row + c0, a);
            st4(row + gm.c + c0, b);
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// One pass produces dx (gradient w.r.t. the activated input) and a per-block partial of dW.
// Each thread owns the output strip (n, ho, wo0..wo0+3) for dW and the input patch rows [ho*S, ho*S+S) x cols
// [wo0*S, wo0*S + 4*S) for dx; the 3x6 window of dy around the strip serves both.
template <int S, int DIL, int PT, int PL>
__global__ void __launch_bounds__(512) dw_bwd_kernel(DwGeom gm, ViewDev in, const float* __restrict__ wgt, GViewDev dy,
                                                     float* __restrict__ dx, float* __restrict__ dwpart, int accumulate) {
    extern __shared__ float4 red[];
    const BlockPos bpos = xcd_block_pos();   // (tile slot, channel group), neighbouring slots on the same XCD / L2
    const int cvi = bpos.y * blockDim.x + threadIdx.x;
    const bool active = cvi < gm.cv;
    const int c0 = cvi * 4;
    ChanCoef ci, co;  // input-side view coefficients, output-side gradient-view coefficients
    ci.affine = in.scale != nullptr;
    co.affine = dy.scale != nullptr;
    ci.s = co.s = f4(1.f);
    ci.t = ci.k1 = ci.k0 = co.t = co.k1 = co.k0 = f4(0.f);
    ci.lo = act_lo(in.act); ci.hi = act_hi(in.act);
    co.lo = co.hi = 0.f;
    if (!co.affine) { dy.y = dy.g; dy.act = SSDSEG_ACT_NONE; }   // identity gradient view, branch-free form
    if (active) {
        if (ci.affine) { ci.s = ld4(in.scale + c0); ci.t = ld4(in.shift + c0); }
        if (co.affine) { co.s = ld4(dy.scale + c0); co.t = ld4(dy.shift + c0); co.k1 = ld4(dy.k1 + c0); co.k0 = ld4(dy.k0 + c0); }
    }
    float4 dwacc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) dwacc[t] = f4(0.f);

    if (active) {
        for (long long tile = (long long)bpos.x * blockDim.y + threadIdx.y; tile < gm.ntiles;
             tile += (long long)gridDim.x * blockDim.y) {
            const int wt = (int)(tile % gm.wtiles);
            const long long r = tile / gm.wtiles;
            const int ho = (int)(r % gm.ho);
            const int n = (int)(r / gm.ho);
            const int wo0 = wt * TW;
            const long long oimg = (long long)n * gm.ho * gm.wo;
            const long long iimg = (long long)n * gm.h * gm.w;

            if (DIL == 1) {
                // ---- dy window rows ho-1..ho+1, cols wo0-1..wo0+TW
                float4 dyw[3][TW + 2];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int hh = ho - 1 + a;
#pragma unroll
                    for (int b = 0; b < TW + 2; ++b) {
                        const int ww = wo0 - 1 + b;
                        dyw[a][b] = load_gview_if(dy, co, (oimg + (long long)hh * gm.wo + ww) * gm.c + c0,
                                                  hh >= 0 && hh < gm.ho && ww >= 0 && ww < gm.wo, c0);
                    }
                }
                // ---- dx over the owned input patch
                if (dx != nullptr) {
                    float4 wk[9];
#pragma unroll
                    for (int t = 0; t < 9; ++t) wk[t] = ld4(wgt + (long long)t * gm.c + c0);
#pragma unroll
                    for (int ir = 0; ir < S; ++ir) {
                        const int hi = ho * S + ir;
                        if (hi >= gm.h) continue;
#pragma unroll
                        for (int ic = 0; ic < TW * S; ++ic) {
                            const int wi = wo0 * S + ic;
                            if (wi >= gm.w) continue;
                            float4 acc = f4(0.f);
#pragma unroll
                            for (int kh = 0; kh < 3; ++kh) {
                                // ho' = (hi + PT - kh) / S must be integral: (ir + PT - kh) % S == 0
                                if (((ir + PT - kh) % S + S) % S != 0) continue;
                                const int ra = ((ir + PT - kh) - (((ir + PT - kh) % S + S) % S)) / S + 1;  // window row, compile-time
#pragma unroll
                                for (int kw = 0; kw < 3; ++kw) {
                                    if (((ic + PL - kw) % S + S) % S != 0) continue;
                                    const int cb = ((ic + PL - kw) - (((ic + PL - kw) % S + S) % S)) / S + 1;  // window col
                                    if (ra >= 0 && ra < 3 && cb >= 0 && cb < TW + 2) fma4(acc, dyw[ra][cb], wk[kh * 3 + kw]);
                                }
                            }
                            float* p = dx + (iimg + (long long)hi * gm.w + wi) * gm.c + c0;
                            if (accumulate) add4(acc, ld4(p));
                            st4(p, acc);
                        }
                    }
                }
                // ---- dW: a-window row by row against the centre row of dy
                constexpr int WC = (TW - 1) * S + 3;
                const int wi0 = wo0 * S - PL;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int hi = ho * S + kh - PT;
                    const bool rowok = hi >= 0 && hi < gm.h;
                    float4 row[WC];
#pragma unroll
                    for (int q = 0; q < WC; ++q) {
                        const int wi = wi0 + q;
                        row[q] = load_view_if(in, ci, (iimg + (long long)hi * gm.w + wi) * gm.c + c0, rowok && wi >= 0 && wi < gm.w, c0);
                    }
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                        for (int j = 0; j < TW; ++j) fma4(dwacc[kh * 3 + kw], row[j * S + kw], dyw[1][j + 1]);
                }
            } else {
                // dilated, stride 1, pads == dilation: direct gathers
                const int d = gm.d;
                float4 wk[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) wk[t] = ld4(wgt + (long long)t * gm.c + c0);
#pragma unroll
                for (int j = 0; j < TW; ++j) {
                    const int wq = wo0 + j;
                    if (wq >= gm.wo) continue;
                    const float4 dyc = load_gview(dy, co, (oimg + (long long)ho * gm.wo + wq) * gm.c + c0);
                    float4 acc = f4(0.f);
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh) {
                        const int hh = ho + gm.pt - kh * d;   // output row feeding dx at input row ho
                        const int hi = ho + kh * d - gm.pt;   // input row feeding dW from output row ho
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            const int ww = wq + gm.pl - kw * d;
                            const int wi = wq + kw * d - gm.pl;
                            if (dx != nullptr && hh >= 0 && hh < gm.ho && ww >= 0 && ww < gm.wo)
                                fma4(acc, load_gview(dy, co, (oimg + (long long)hh * gm.wo + ww) * gm.c + c0), wk[kh * 3 + kw]);
                            if (hi >= 0 && hi < gm.h && wi >= 0 && wi < gm.w)
                                fma4(dwacc[kh * 3 + kw], load_view(in, ci, (iimg + (long long)hi * gm.w + wi) * gm.c + c0), dyc);
                        }
                    }
                    if (dx != nullptr) {
                        float* p = dx + (iimg + (long long)ho * gm.w + wq) * gm.c + c0;
                        if (accumulate) add4(acc, ld4(p));
                        st4(p, acc);
                    }
                }
            }
        }
    }
    // ---- block partial of dW: [gridDim.x][9][c]
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float4 v = reduce_over_y(dwacc[t], red);
        if (threadIdx.y == 0 && active) st4(dwpart + ((long long)bpos.x * 9 + t) * gm.c + c0, v);
    }
}

struct DwLaunch { dim3 grid, block; size_t lds; };

// sizes and pads of a call: what every family needs, and the kernel argument of all but the marching kernels
DwGeom dw_geom(int n, int h, int w, int c, int stride, int dilation) {
    DwGeom g;
    g.n = n; g.h = h; g.w = w; g.c = c; g.s = stride; g.d = dilation;
    same_pad(h, 3, stride, dilation, &g.ho, &g.pt);
    same_pad(w, 3, stride, dilation, &g.wo, &g.pl);
    g.cv = c / 4;
    g.wtiles = cdiv(g.wo, TW);
    g.ntiles = (long long)n * g.ho * g.wtiles;
    return g;
}

// launch of the register-window and gather kernels
DwLaunch reg_launch(const DwGeom& g) {
    int bx = g.cv < 256 ? g.cv : 256;
    int by = 512 / bx;
    if (by > 64) by = 64;
    if (by < 1) by = 1;
    long long want = (g.ntiles + by - 1) / by;
    int gx = (int)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    if (gx < 1) gx = 1;
    gx = (gx + 7) & ~7;   // multiple of 8 for the XCD remap (surplus blocks find no tile and write zero partial rows)
    return DwLaunch{dim3(gx, cdiv(g.cv, bx), 1), dim3(bx, by, 1), (size_t)bx * by * sizeof(float4)};
}

}  // namespace

#include "dwconv_lds.h"
#include "dwconv_march.h"

#include <stdarg.h>
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------ the plan of a call
// Everything the host decides about one call, decided ONCE: the kernel family, that family's geometry and launch, the partial
// rows it writes and the template flags of its kernel.  ssdseg_dwconv_parts, the zeroing of surplus statistics rows and the
// launches all read it.  The switches are read on every call, not cached: the parity tests flip them between calls.
enum DwFamily {
    DW_MARCH,    // column-marching kernels (dwconv_march.h): the forward at both strides, the stride-1 backward (dilated: sub-grids)
    DW_MARCH2,   // the stride-2 backward march
    DW_LDS,      // LDS-tiled kernels (dwconv_lds.h), dense taps
    DW_REG,      // register-window backward, dense taps
    DW_GATHER    // direct gathers of the dilated convs (the DIL == 0 form of the register-window kernels)
};
struct DwPlan {
    DwFamily family;
    DwGeom g;           // every family: sizes and pads
    MarchGeom mg;       // DW_MARCH backward
    March2Geom mg2;     // DW_MARCH forward, DW_MARCH2
    DwLaunch l;
    int rows;           // partial rows the kernel writes (one per block along grid.x): BatchNorm statistics forward, dW backward
    bool fuse, acc, wfull;   // backward marches: BNFUSE, ACC and WFULL of the kernel
};

// the marching kernels address with 32-bit byte offsets
bool dw_march_fits(int n, int h, int w, int c) { return (long long)n * h * w * c < (1LL << 30); }

// forward plan of one family (ssdseg_dwconv_parts asks for both candidates of a layer, a call for the one it runs)
DwPlan dw_fwd_plan(DwFamily family, int n, int h, int w, int c, int stride, int dilation) {
    DwPlan p{};
    p.family = family;
    p.g = dw_geom(n, h, w, c, stride, dilation);
    if (family == DW_LDS) p.l = stride == 1 ? lds_launch<1>(p.g, true) : lds_launch<2>(p.g, true);
    else if (family != DW_MARCH) p.l = reg_launch(p.g);
    else {
        p.mg2 = March2Geom{n, h, w, c, p.g.ho, p.g.wo};
        p.l = march_geometry(&p.mg2, n, p.g.ho, p.g.wo, c, stride == 1 ? 4 : 2, 2, 4096, dilation);
        p.mg2.depth2 = !env_is("SSDSEG_DW_FWD_DEPTH", '1');
    }
    p.rows = (int)p.l.grid.x;
    return p;
}

// forward family: column-marching for every conv whose tensors fit 32-bit byte offsets (SSDSEG_DW_FWD=lds keeps the LDS-tiled
// kernels, SSDSEG_DW_ATROUS=gather the direct-gather kernel of the dilated convs: A/B measurements, parity tests)
DwFamily dw_fwd_family(int n, int h, int w, int c, int dilation) {
    const bool lds = env_pick("SSDSEG_DW_FWD", {"lds"}) != 0;
    const bool atrous_ok = env_pick("SSDSEG_DW_ATROUS", {"gather"}) == 0;
    if (!lds && (dilation == 1 || atrous_ok) && dw_march_fits(n, h, w, c)) return DW_MARCH;
    return dilation == 1 ? DW_LDS : DW_GATHER;
}

// rows of the BatchNorm statistics table of a layer: the larger count of the two forward kernels that can take it, whatever the
// switches say when the table is allocated (`have`: the plan the caller has made already)
int dw_fwd_table_rows(int n, int h, int w, int c, int stride, int dilation, const DwPlan* have) {
    int rows = 0;
    for (DwFamily f : {DW_MARCH, dilation == 1 ? DW_LDS : DW_GATHER}) {
        if (f == DW_MARCH && !dw_march_fits(n, h, w, c)) continue;
        const int r = have != nullptr && have->family == f ? have->rows : dw_fwd_plan(f, n, h, w, c, stride, dilation).rows;
        if (r > rows) rows = r;
    }
    return rows;
}

// backward plan.  SSDSEG_DW_BWD=march|lds|reg forces one kernel family (A/B measurements); default: measured best per shape
DwPlan dw_bwd_plan(int n, int h, int w, int c, int stride, int dilation, bool has_dx, bool accumulate, bool has_bn) {
    DwPlan p{};
    p.g = dw_geom(n, h, w, c, stride, dilation);
    const int choice = env_pick("SSDSEG_DW_BWD", {"march", "lds", "reg"});
    const bool march = (choice == 0 || choice == 1) && dw_march_fits(n, h, w, c);
    // atrous (stride 1, SAME: pad == dilation): dilation^2 interleaved dense convs through the same marching kernel
    // (SSDSEG_DW_ATROUS=gather keeps the direct-gather kernel: nine two-tensor gathers per output pixel, 0.5 TB/s)
    const bool atrous_march = dilation > 1 && env_pick("SSDSEG_DW_ATROUS", {"gather"}) == 0 && p.g.pt == dilation && p.g.pl == dilation &&
                              p.g.ho == h && p.g.wo == w;
    if (march && stride == 1 && (dilation == 1 || atrous_march)) {
        p.family = DW_MARCH;
        p.mg = MarchGeom{n, h, w, c};
        p.l = march_geometry(&p.mg, n, h, w, c, MTW, 11, march_min_waves(), dilation);
        p.fuse = has_bn && dilation == 1 && has_dx;   // (with accumulate: this conv is the LAST writer of dx)
        p.acc = accumulate;
        p.wfull = w % MTW == 0 && dilation == 1;
    } else if (march && stride == 2 && dilation == 1) {
        p.family = DW_MARCH2;
        p.mg2 = March2Geom{n, h, w, c, p.g.ho, p.g.wo};
        p.l = march_geometry(&p.mg2, n, p.g.ho, p.g.wo, c, 2, 11, 4096, 1);
        p.fuse = has_bn && has_dx;
        p.acc = accumulate && has_dx;
    } else if (dilation == 1 && stride == 1 && (choice == 2 || (choice != 3 && c <= 160))) {
        // measured on MI355X (profiles/): the fused LDS backward wins for stride 1 with few channel groups (big early layers,
        // decoder); with many channel groups or stride 2 its 256-VGPR footprint loses to the register-window kernel
        p.family = DW_LDS;
        p.l = lds_launch<1>(p.g, false);
    } else {
        p.family = dilation == 1 ? DW_REG : DW_GATHER;
        p.l = reg_launch(p.g);
    }
    p.rows = (int)p.l.grid.x;
    return p;
}

// ------------------------------------------------------------------------------------------------ launches
// run-time flags -> template arguments (the idiom of for_width in gemm_internal.h): f is a generic lambda over one
// std::bool_constant per flag, and rules the combinations no plan names out with `if constexpr`, so that they are not compiled
template <class F>
int for_flags(F&& f) { return f(); }
template <class F, class... Rest>
int for_flags(F&& f, bool flag, Rest... rest) {
    auto bind = [&](auto B) { return for_flags([&](auto... more) { return f(B, more...); }, rest...); };
    return flag ? bind(std::true_type{}) : bind(std::false_type{});
}
#define FLAG(B) (decltype(B)::value)

int dw_no_kernel(const char* which) {
    ssdseg_set_error("%s: the plan names an instantiation that does not exist", which);
    return SSDSEG_EINVAL(0);
}

// name of a template instance in the timing registry, spelled as SSDSEG_LAUNCH stringifies a literal one -- parentheses
// included: "(dw_bwd_march_kernel<true, true, false, false>)" (bench.py and profiles/ key on these).  Built only while timing is on.
const char* dw_kname(const ssdseg_ctx* ctx, const char* fmt, ...) {
    if (!ctx->timing) return "";
    char buf[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return ssdseg_intern(buf);
}
const char* tf(bool b) { return b ? "true" : "false"; }

struct BnFuse {   // BatchNorm-backward reduction of the layer feeding this depthwise conv, fused into its backward
    const float* mean;
    const float* invstd;
    float *dgamma, *dbeta, *k1, *k0;
};

int dw_bwd_impl(ssdseg_ctx* ctx, const ssdseg_view* in, const float* w, const ssdseg_gview* dy, float* dx, float* dw, int n, int h,
                int wdt, int c, int stride, int dilation, int accumulate, const BnFuse* bn, bool* bn_done) {
    const DwPlan p = dw_bwd_plan(n, h, wdt, c, stride, dilation, dx != nullptr, accumulate != 0, bn != nullptr);
    const DwGeom& g = p.g;
    const DwLaunch& l = p.l;
    ViewDev v{in->x, in->scale, in->shift, in->act};
    GViewDev gv{dy->g, dy->y, dy->scale, dy->shift, dy->k1, dy->k0, dy->act};
    // algorithmic traffic, SURVEY.md 8(d): 4 * (2*X + Y + 18*C) -- read X, read dY, write dX, read W, write dW.  A BatchNorm-backward
    // gradient view is formed from TWO tensors (g and the raw forward output y): the second one is what this design reads on top
    // of 8(d)'s ideal and is reported separately (`view_bytes`), never inside the roofline's algorithmic bytes.
    const double cost_bytes = 4.0 * (2.0 * n * h * wdt * c + (double)n * g.ho * g.wo * c + 18.0 * c);
    ctx->timing_view_bytes = dy->scale != nullptr ? 4.0 * n * g.ho * g.wo * c : 0.0;
    const double cost_flops = 36.0 * n * g.ho * g.wo * c;
    if (bn_done) *bn_done = false;
    // partial table: [rows][9][c] of dW, and behind it the marching kernels' [rows][2][c] of the fused BatchNorm sums (requested
    // by every march, fused or not)
    const bool march = p.family == DW_MARCH || p.family == DW_MARCH2;
    void* ws;
    int rc = ssdseg_partials(ctx, (size_t)p.rows * (march ? 11 : 9) * c * sizeof(float), &ws);
    if (rc) return rc;
    float* part = (float*)ws;
    float* bnpart = p.fuse ? part + (size_t)p.rows * 9 * c : nullptr;
    const float* mean = p.fuse ? bn->mean : nullptr;
    const float* invstd = p.fuse ? bn->invstd : nullptr;
    if (p.family == DW_MARCH) {
        rc = for_flags([&](auto BN, auto WF, auto AC, auto DIL) {
            constexpr bool exists = !(FLAG(DIL) && (FLAG(BN) || FLAG(WF)));     // (the dilated march: neither fused nor WFULL)
            if constexpr (exists)
                SSDSEG_LAUNCH_NAMED(ctx, dw_kname(ctx, "(dw_bwd_march_kernel<%s, %s, %s, %s>)", tf(FLAG(BN)), tf(FLAG(WF)), tf(FLAG(AC)), tf(FLAG(DIL))),
                                    cost_bytes, cost_flops, (dw_bwd_march_kernel<FLAG(BN), FLAG(WF), FLAG(AC), FLAG(DIL)>), l.grid, l.block, l.lds,
                                    p.mg, v, w, gv, dx, part, accumulate, mean, invstd, bnpart);
            return exists ? 0 : dw_no_kernel("dw_bwd_march_kernel");
        }, p.fuse, p.wfull, p.acc, dilation > 1);
    } else if (p.family == DW_MARCH2) {
        rc = for_flags([&](auto BN, auto PT, auto PL, auto AC) {
            SSDSEG_LAUNCH_NAMED(ctx, dw_kname(ctx, "(dw_bwd_march2_kernel<%s, %d, %d, %s>)", tf(FLAG(BN)), (int)FLAG(PT), (int)FLAG(PL), tf(FLAG(AC))),
                                cost_bytes, cost_flops, (dw_bwd_march2_kernel<FLAG(BN), FLAG(PT), FLAG(PL), FLAG(AC)>), l.grid, l.block, l.lds,
                                p.mg2, v, w, gv, dx, part, accumulate, mean, invstd, bnpart);
            return 0;
        }, p.fuse, g.pt != 0, g.pl != 0, p.acc);
    } else if (p.family == DW_LDS) {
        SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, (dw_bwd_lds_kernel<1, 1, 1>), l.grid, l.block, l.lds, g, v, w, gv, dx, part, accumulate);
    } else {
        // <S, DIL, PT, PL>: gather <1, 0, 0, 0> (pads at run time) | stride 1 <1, 1, 1, 1> | stride 2 <2, 1, pt, pl>
        const bool dense = p.family == DW_REG;
        rc = for_flags([&](auto S2, auto DENSE, auto PT, auto PL) {
            constexpr bool exists = FLAG(DENSE) ? (FLAG(S2) || (FLAG(PT) && FLAG(PL))) : (!FLAG(S2) && !FLAG(PT) && !FLAG(PL));
            constexpr int S = FLAG(S2) ? 2 : 1;
            if constexpr (exists)
                SSDSEG_LAUNCH_NAMED(ctx, dw_kname(ctx, "(dw_bwd_kernel<%d, %d, %d, %d>)", S, (int)FLAG(DENSE), (int)FLAG(PT), (int)FLAG(PL)), cost_bytes,
                                    cost_flops, (dw_bwd_kernel<S, FLAG(DENSE), FLAG(PT), FLAG(PL)>), l.grid, l.block, l.lds, g, v, w, gv, dx, part,
                                    accumulate);
            return exists ? 0 : dw_no_kernel("dw_bwd_kernel");
        }, stride == 2, dense, dense && (stride == 1 || g.pt != 0), dense && (stride == 1 || g.pl != 0));
    }
    if (rc) return rc;
    SSDSEG_LAUNCH_CHECK();
    rc = ssdseg_colsum(ctx, part, p.rows, 9LL * c, dw);
    if (rc || !p.fuse) return rc;
    *bn_done = true;
    return ssdseg_bn_bwd_finalize_launch(ctx, bnpart, p.rows, c, (double)n * h * wdt, in->scale, bn->mean, bn->invstd, bn->dgamma,
                                         bn->dbeta, bn->k1, bn->k0);
}

}  // namespace

extern "C" {

int ssdseg_dwconv_parts(int n, int h, int w, int c, int stride, int dilation, int* nparts_host) {
    SSDSEG_ARG(n > 0 && h > 0 && w > 0, 1);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 4);
    SSDSEG_ARG(stride == 1 || stride == 2, 5);
    SSDSEG_ARG(dilation >= 1 && (dilation == 1 || stride == 1), 6);
    SSDSEG_ARG(nparts_host != nullptr, 7);
    // (ssdseg_dwconv_fwd zeroes the rows the launched kernel does not write)
    *nparts_host = dw_fwd_table_rows(n, h, w, c, stride, dilation, nullptr);
    return 0;
}

int ssdseg_dwconv_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, const float* w, float* y, int n, int h, int wdt, int c,
                      int stride, int dilation, float* stats) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr, 2);
    SSDSEG_ARG(w != nullptr, 3);
    SSDSEG_ARG(y != nullptr, 4);
    SSDSEG_ARG(n > 0, 5);
    SSDSEG_ARG(h > 0, 6);
    SSDSEG_ARG(wdt > 0, 7);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 8);
    SSDSEG_ARG(stride == 1 || stride == 2, 9);
    SSDSEG_ARG(dilation >= 1 && (dilation == 1 || stride == 1), 10);
    SSDSEG_ARG((in->scale == nullptr) == (in->shift == nullptr), 2);
    const DwPlan p = dw_fwd_plan(dw_fwd_family(n, h, wdt, c, dilation), n, h, wdt, c, stride, dilation);
    const DwGeom& g = p.g;
    const DwLaunch& l = p.l;
    ViewDev v{in->x, in->scale, in->shift, in->act};
    // algorithmic traffic: read X, write Y, read W
    const double cost_bytes = 4.0 * ((double)n * h * wdt * c + (double)n * g.ho * g.wo * c + 9.0 * c);
    const double cost_flops = 18.0 * n * g.ho * g.wo * c;
    if (stats != nullptr) {      // the table is sized for the largest candidate (ssdseg_dwconv_parts): the rows this launch does not write are zero
        const int nparts = dw_fwd_table_rows(n, h, wdt, c, stride, dilation, &p);
        if (nparts > p.rows) SSDSEG_HIP(hipMemsetAsync(stats + (size_t)p.rows * 2 * c, 0, (size_t)(nparts - p.rows) * 2 * c * sizeof(float), ctx->stream));
    }
    int rc = 0;
    if (p.family == DW_MARCH) {
        // <S, PT, PL, DIL, D2>: stride 1 <1, 1, 1, dilated, two rows ahead (dense taps only)> | stride 2 <2, pt, pl, false, false>
        const bool s2 = stride == 2, dil = dilation > 1;
        rc = for_flags([&](auto S2, auto PT, auto PL, auto DIL, auto D2) {
            constexpr bool exists = FLAG(S2) ? (!FLAG(DIL) && !FLAG(D2)) : (FLAG(PT) && FLAG(PL) && !(FLAG(DIL) && FLAG(D2)));
            constexpr int S = FLAG(S2) ? 2 : 1;
            if constexpr (exists)      // (D2 = false is the template's default and is not spelled in the name)
                SSDSEG_LAUNCH_NAMED(ctx, dw_kname(ctx, "(dw_fwd_march_kernel<%d, %d, %d, %s%s>)", S, (int)FLAG(PT), (int)FLAG(PL), tf(FLAG(DIL)), FLAG(D2) ? ", true" : ""),
                                    cost_bytes, cost_flops, (dw_fwd_march_kernel<S, FLAG(PT), FLAG(PL), FLAG(DIL), FLAG(D2)>), l.grid, l.block, l.lds, p.mg2,
                                    v, w, y, stats);
            return exists ? 0 : dw_no_kernel("dw_fwd_march_kernel");
        }, s2, !s2 || g.pt != 0, !s2 || g.pl != 0, dil, !s2 && !dil && p.mg2.depth2 != 0);
    } else if (p.family == DW_LDS) {
        rc = for_flags([&](auto S2) {
            constexpr int S = FLAG(S2) ? 2 : 1;
            SSDSEG_LAUNCH_NAMED(ctx, dw_kname(ctx, "(dw_fwd_lds_kernel<%d>)", S), cost_bytes, cost_flops, (dw_fwd_lds_kernel<S>), l.grid, l.block, l.lds, g, v, w,
                                y, stats);
            return 0;
        }, stride == 2);
    } else {
        SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, (dw_fwd_kernel<1, 0>), l.grid, l.block, l.lds, g, v, w, y, stats);
    }
    if (rc) return rc;
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_dwconv_bwd(ssdseg_ctx* ctx, const ssdseg_view* in, const float* w, const ssdseg_gview* dy, float* dx,
                      float* dw, int n, int h, int wdt, int c, int stride, int dilation, int accumulate) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr, 2);
    SSDSEG_ARG((in->scale == nullptr) == (in->shift == nullptr), 2);
    SSDSEG_ARG(w != nullptr, 3);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 4);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 4);
    SSDSEG_ARG(dw != nullptr, 6);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 7);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 10);
    SSDSEG_ARG(stride == 1 || stride == 2, 11);
    SSDSEG_ARG(dilation >= 1 && (dilation == 1 || stride == 1), 12);
    return dw_bwd_impl(ctx, in, w, dy, dx, dw, n, h, wdt, c, stride, dilation, accumulate, nullptr, nullptr);
}

int ssdseg_dwconv_bwd_bn(ssdseg_ctx* ctx, const ssdseg_view* in, const float* w, const ssdseg_gview* dy, float* dx, float* dw, int n,
                         int h, int wdt, int c, int stride, int dilation, int accumulate, const float* in_mean, const float* in_invstd,
                         float* in_dgamma, float* in_dbeta, float* in_k1, float* in_k0) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && in->scale != nullptr && in->shift != nullptr, 2);
    SSDSEG_ARG(w != nullptr, 3);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 4);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 4);
    SSDSEG_ARG(dx != nullptr, 5);
    SSDSEG_ARG(dw != nullptr, 6);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 7);
    SSDSEG_ARG((long long)n * h * wdt <= 0x7fffffffLL, 7);   // (the unfused reduction counts pixels in an int)
    SSDSEG_ARG(c > 0 && c % 4 == 0, 10);
    SSDSEG_ARG(stride == 1 || stride == 2, 11);
    SSDSEG_ARG(dilation >= 1 && (dilation == 1 || stride == 1), 12);
    SSDSEG_ARG(in_mean != nullptr && in_invstd != nullptr, 14);
    SSDSEG_ARG(in_k1 != nullptr && in_k0 != nullptr, 18);
    const BnFuse bn{in_mean, in_invstd, in_dgamma, in_dbeta, in_k1, in_k0};
    bool done = false;
    int rc = dw_bwd_impl(ctx, in, w, dy, dx, dw, n, h, wdt, c, stride, dilation, accumulate, &bn, &done);
    if (rc || done) return rc;
    // shapes without a fused kernel: the same reduction as a separate pass over (dx, x)
    return ssdseg_bn_bwd_reduce(ctx, dx, c, in->x, c, n * h * wdt, c, in->scale, in->shift, in_mean, in_invstd, in->act, in_dgamma, in_dbeta,
                                in_k1, in_k0);
}

}  // extern "C"
