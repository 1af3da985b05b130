// What gemm.hip, pw_wgrad.hip and the units built on their kernels (conv3.hip, stem.hip) share: the argument structs of
// gemm_rowA_kernel / gemm_wgrad_kernel, the tile constants, the column-tile rule and the few launch helpers that cross a unit
// boundary.  Hidden helpers like ssdseg_colsum: exported by the library, not part of include/ssdseg.h.  gemm_rowA_kernel is
// instantiated in gemm.hip alone, gemm_wgrad_kernel in pw_wgrad.hip alone.
#pragma once
#include "common.h"

#include <type_traits>

// gemm_rowA_kernel / gemm_wres_kernel tile: 128 rows per block, 32 reduction channels per step, staged as [128][32 + 4]
constexpr int BM = 128;
constexpr int BK = 32;
constexpr int AS = BK + 4;
// rows from which the occupancy-limited gemm_rowA_kernel instantiations run; the weight gradient's "long M" by the same count
constexpr int ROWA_OCC_ROWS = 150000;

// Column-tile width in 32-col MFMA tiles.  `row_blocks` = how many blocks the launch has per column tile.
// Among the widths that still give the chip >= 2 blocks per CU, take the one wasting the fewest padded columns (ties ->
// wider: more reuse of the streamed operand per block); if no width reaches that, take the one with the most blocks
// (the 15x20 / 8x10 layers have only 75 / 20 row tiles: a 160-wide tile would leave 180 of 256 CUs idle).
inline int pick_wn(int n, long long row_blocks) {
    int best = 1;
    long long best_pad = -1, best_blocks = -1;
    bool best_full = false;
    for (int wn = 1; wn <= 5; ++wn) {
        const long long tiles = (n + 32 * wn - 1) / (32 * wn);
        const long long pad = tiles * 32 * wn, blocks = tiles * row_blocks;
        const bool full = blocks >= 512;
        bool take;
        if (best_pad < 0) take = true;
        else if (full != best_full) take = full;
        else if (full) take = pad <= best_pad;
        else take = blocks > best_blocks || (blocks == best_blocks && pad <= best_pad);
        if (take) { best = wn; best_pad = pad; best_blocks = blocks; best_full = full; }
    }
    return best;
}

// ---- run-time tile width (and occupancy flag) -> template arguments.  `f` is a generic lambda over std::integral_constant;
// widths LO .. HI - 1 name themselves, HI is the catch-all, and only the widths of the range are instantiated:
//   float4 epilogue 2..5 | plain, resident, BN epilogue, weight gradient 1..5 | fused dx + dW (the width is the chunk count NT) 1..6
template <int LO, int HI, class F>
int for_width(int w, F&& f) {
    if constexpr (LO < HI) {
        if (w == LO) return f(std::integral_constant<int, LO>{});
        return for_width<LO + 1, HI>(w, f);
    } else {
        return f(std::integral_constant<int, HI>{});
    }
}
template <int LO, int HI, class F>
int for_width_occ(int w, bool occ, F&& f) {
    return for_width<LO, HI>(w, [&](auto W) { return occ ? f(W, std::integral_constant<int, 1>{}) : f(W, std::integral_constant<int, 0>{}); });
}

struct ssdseg_rowa_args {
    const float* a0;   // x (fwd) | g (bwd_data)
    const float* a1;   // unused  | y
    const float* cs;   // per-reduction-channel coefficients (nullable -> identity)
    const float* ct;
    const float* ck1;
    const float* ck0;
    int act;
    int lda;
    const float* b;
    int ldb;
    float* out;
    int ldo;
    const float* residual;
    int ldr;
    int accumulate;
    float* stats;
    int I, R, J;
    // dense 3x3 stride-1 SAME convolution as implicit GEMM (CONV kernels): the reduction axis is (tap, channel) with
    // convC channels per tap, row m = (n, h, w) reads the streamed operand at (h + sign*(kh-1), w + sign*(kw-1))
    int convH, convW, convC, convSign;
    // stem (LD == 2): 3x3 stride-2 SAME conv on a 3-channel image as implicit GEMM with R = 27 = (kh, kw, ci); row m =
    // (n, ho, wo) over convH x convW OUTPUT pixels reads image (2*ho + kh - stemPt, 2*wo + kw - stemPl, ci) of a
    // stemH x stemW image, rescaled on load (x*stemScale + stemOffset; padding stays 0).  bias: optional, added in the epilogue.
    int stemH, stemW, stemPt, stemPl;
    float stemScale, stemOffset;
    const float* bias;
    // fused backward (NT > 0, MODE 1): the layer's INPUT view x[I][J] (a = act(xs*x + xt)) and the per-block partial slabs of
    // dW[J][R] = sum_m a[m][j] * dy[m][r]  ([gridDim.y][J][R]); the dy tile already sits in LDS for the dx product
    const float* xw;
    const float* xws;
    const float* xwt;
    int xwact, ldxw;
    float* wpart;
    // BNE (MODE 1): BatchNorm backward of the producer of this conv's INPUT, fused into the (LDS-transposed, float4) epilogue:
    // raw input bn_y[I][J] (ld ldby), that BN's scale/shift/mean/invstd/activation; bnpart: [gridDim.y][2][J] partial rows of
    // (sum mask*dx, sum mask*dx*xhat)
    const float* bn_y;
    const float* bn_s;
    const float* bn_t;
    const float* bn_mean;
    const float* bn_istd;
    int bn_act, ldby;
    float* bnpart;
};

struct ssdseg_wgrad_args {
    const float* x;  // view over [M][K]
    const float* xs;
    const float* xt;
    int xact;
    int ldx;
    const float* g;  // gview over [M][N]
    const float* y;
    const float* gs;
    const float* gt;
    const float* gk1;
    const float* gk0;
    int gact;
    int ldy;
    float* part;  // [P][K][N]
    int M, K, N;
    int rows_per_split;
    // one tap of a dense 3x3 conv: row m = (n, h, w) reads x at (h + dh, w + dw); convH == 0 -> plain GEMM
    int convH, convW, dh, dw;
    // stem: x is the 3-channel image, row m = (n, ho, wo) over convH x convW output pixels, k = (kh, kw, ci) (see ssdseg_rowa_args)
    int stem, stemH, stemW, stemPt, stemPl;
    float stemScale, stemOffset;
};

extern "C" {
// ---- gemm.hip
// row-tile slots per column tile of a gemm_rowA_kernel launch == partial rows of the BatchNorm statistics table it writes
int ssdseg_rowA_grid_y(int rows, int cols);
// gemm_rowA_kernel over the dense 3x3 gather (LD = 1), forward and input gradient, and over the stem gather (LD = 2)
int ssdseg_rowA_conv3_fwd(ssdseg_ctx* ctx, const ssdseg_rowa_args& a);
int ssdseg_rowA_conv3_bwd_data(ssdseg_ctx* ctx, const ssdseg_rowa_args& a);
int ssdseg_rowA_stem_fwd(ssdseg_ctx* ctx, const ssdseg_rowa_args& a);
// ---- pw_wgrad.hip
// picks the tile shape / split count for dw[k][n] = sum_m x[m][k]*dy[m][n], launches, reduces the split partials
int ssdseg_wgrad_run(ssdseg_ctx* ctx, const ssdseg_wgrad_args& a, float* dw);
// ---- gemm.hip
// dx = dy * w^T plus the BatchNormalization backward of the layer that feeds this conv (sums in the GEMM epilogue)
int ssdseg_pwconv_bwd_data_bn(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy, const float* w, float* dx,
                              int lddx, int m, int k, int n, const float* in_mean, const float* in_invstd, float* in_dgamma,
                              float* in_dbeta, float* in_k1, float* in_k0);
// ---- conv3.hip
// W[tap][c][n] -> Wt[tap][n][c] for `taps` matrices (conv3_transpose_w_kernel; the pointwise tile GEMM's forward uses it with taps = 1)
int ssdseg_transpose_w(ssdseg_ctx* ctx, const float* w, float* wt, int cin, int cout, int taps);
// ---- conv3n.hip: the narrow 3x3 conv's input gradient + fused BatchNorm sums as a streaming kernel (cin == 256, cout == 4)
bool ssdseg_conv3n_direct_takes(int cin, int cout, int ldx);
int ssdseg_conv3n_bwd_bn_direct(ssdseg_ctx* ctx, const ssdseg_view* in, const ssdseg_gview* dy, const float* w, float* dx, int ldx, int n, int h,
                                int wdt, const float* in_mean, const float* in_invstd, float* in_dgamma, float* in_dbeta, float* in_k1,
                                float* in_k0);
}
