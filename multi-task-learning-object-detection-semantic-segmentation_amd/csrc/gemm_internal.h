// What the units built on the GEMM kernels (conv3.hip, stem.hip) and gemm.hip share: the argument structs of gemm_rowA_kernel /
// gemm_wgrad_kernel and the few launch helpers that cross the unit boundary.  Hidden helpers like ssdseg_colsum: exported by the
// library, not part of include/ssdseg.h.  The kernels are instantiated in gemm.hip alone.
#pragma once
#include "common.h"

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
// picks the tile shape / split count for dw[k][n] = sum_m x[m][k]*dy[m][n], launches, reduces the split partials
int ssdseg_wgrad_run(ssdseg_ctx* ctx, const ssdseg_wgrad_args& a, float* dw);
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
