// Pooling and resize kernels of the DeepLabV3+ head (HBM-bound, float4 over the channel axis, NHWC):
//   GlobalAveragePooling2D keepdims                (reference blocks.py:57)
//   UpSampling2D(bilinear), half-pixel centres     (reference blocks.py:61,104,129; semantics SURVEY.md App. B.5)
#include "lerp_softmax.h"

namespace {

// ------------------------------------------------------------------------------------------------ GAP
// one block per (image, 64-channel-vector group); threads (cv, y) walk the pixels, fixed-order reduction over y
// Sum over the `hw` pixels of "image" blockIdx.x (= one of the `chunks` equal slices of a real image when the caller splits
// the reduction so that n * chunks blocks fill the chip): out[blockIdx.x][c] = mul * sum_p act(s*x + t).  x rows are `ldx` apart.
__global__ void __launch_bounds__(512) gap_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, int act, float* __restrict__ out, int hw, int c,
                                                      float mul) {
    extern __shared__ float4 red[];
    const int cv = c / 4;
    const int cvi = blockIdx.y * blockDim.x + threadIdx.x;
    const int n = blockIdx.x;
    float4 acc = f4(0.f);
    const bool aff = scale != nullptr;
    if (cvi < cv) {
        float4 s = f4(0.f), t = f4(0.f);
        if (aff) { s = ld4(scale + cvi * 4); t = ld4(shift + cvi * 4); }
        for (int p = threadIdx.y; p < hw; p += blockDim.y) add4(acc, view_apply4(ld4(x + ((long long)n * hw + p) * ldx + cvi * 4), s, t, aff, act));
    }
    red[threadIdx.y * blockDim.x + threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.y == 0 && cvi < cv) {
        float4 r = f4(0.f);
        for (int y = 0; y < (int)blockDim.y; ++y) add4(r, red[y * blockDim.x + threadIdx.x]);
        st4(out + (long long)n * c + cvi * 4, make_float4(r.x * mul, r.y * mul, r.z * mul, r.w * mul));
    }
}

// second stage of a split pixel sum: out[n][.] (row stride ldo) = sum_k part[n][k][.] in fixed order (+ previous contents)
__global__ void chunk_sum_kernel(const float* __restrict__ part, int chunks, int cv, float* __restrict__ out, int ldo, int n, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * cv) return;
    const int img = i / cv, c4 = i - img * cv;
    float4 r = f4(0.f);
    for (int k = 0; k < chunks; ++k) add4(r, ld4(part + ((long long)(img * chunks + k) * cv + c4) * 4));
    float* o = out + (long long)img * ldo + c4 * 4;
    if (accumulate) add4(r, ld4(o));
    st4(o, r);
}

// host side of the (optionally split) pixel sum: out[n][c] (row stride ldo) = mul * sum over the hw pixels of each image
int pixel_sum(ssdseg_ctx* ctx, const float* x, int ldx, const float* scale, const float* shift, int act, float* out, int ldo, int n, int hw,
              int c, float mul, int accumulate, double cost_bytes) {
    const int cv = c / 4;
    const int bx = cv < 128 ? cv : 128;
    int chunks = 1;   // equal slices only (deterministic, no ragged tail): the largest divisor of hw that still leaves >= 64 pixels
    for (int k = 16; k >= 2; --k)
        if (hw % k == 0 && hw / k >= 64 && n * k <= 1024) { chunks = k; break; }
    const int hwc = hw / chunks;
    int by = 512 / bx;
    if (by > hwc) by = hwc;
    if (by < 1) by = 1;
    if (chunks == 1 && !accumulate && ldo == c) {
        SSDSEG_LAUNCH(ctx, cost_bytes, 0.0, gap_fwd_kernel, dim3(n, cdiv(cv, bx)), dim3(bx, by), (size_t)bx * by * sizeof(float4), x, ldx, scale,
                      shift, act, out, hw, c, mul);
        SSDSEG_LAUNCH_CHECK();
        return 0;
    }
    void* ws;
    int rc = ssdseg_workspace(ctx, (size_t)n * chunks * c * sizeof(float), &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, cost_bytes, 0.0, gap_fwd_kernel, dim3(n * chunks, cdiv(cv, bx)), dim3(bx, by), (size_t)bx * by * sizeof(float4), x, ldx,
                  scale, shift, act, (float*)ws, hwc, c, mul);
    SSDSEG_LAUNCH_CHECK();
    SSDSEG_LAUNCH(ctx, 4.0 * n * (chunks + 1) * c, 0.0, chunk_sum_kernel, dim3(cdiv(n * cv, 256)), dim3(256), 0, (const float*)ws, chunks, cv, out,
                  ldo, n, accumulate);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

__global__ void gap_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, int n, int hw, int cv, int accumulate) {
    const long long total = (long long)n * hw * cv;
    const float inv = 1.f / (float)hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % cv);
        const long long img = i / ((long long)hw * cv);
        float4 v = ld4(g + (img * cv + c4) * 4);
        v = make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
        if (accumulate) add4(v, ld4(dx + i * 4));
        st4(dx + i * 4, v);
    }
}

// ------------------------------------------------------------------------------------------------ bilinear
__global__ void bilinear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                    int ldx, float* __restrict__ out, int ldo, int n, int h, int w, int cv, int fy, int fx, int pad) {
    const int ho = h * fy, wo = w * fx;
    const int hp = ho + 2 * pad, wp = wo + 2 * pad;       // pad = 1: the output is the interior of a bordered [n][ho+2][wo+2] tensor
    const long long total = (long long)n * ho * wo * cv;
    const bool aff = scale != nullptr;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cv) * 4;
        long long r = i / cv;
        const int ox = (int)(r % wo); r /= wo;
        const int oy = (int)(r % ho);
        const long long img = r / ho;
        const Lerp ly = lerp_of(oy, h, ify), lx = lerp_of(ox, w, ifx);
        float4 s = f4(0.f), t = f4(0.f);
        if (aff) { s = ld4(scale + c0); t = ld4(shift + c0); }
        const float* base = x + img * h * w * ldx + c0;
        const float4 v00 = view_apply4(ld4(base + ((long long)ly.i0 * w + lx.i0) * ldx), s, t, aff, act);
        const float4 v01 = view_apply4(ld4(base + ((long long)ly.i0 * w + lx.i1) * ldx), s, t, aff, act);
        const float4 v10 = view_apply4(ld4(base + ((long long)ly.i1 * w + lx.i0) * ldx), s, t, aff, act);
        const float4 v11 = view_apply4(ld4(base + ((long long)ly.i1 * w + lx.i1) * ldx), s, t, aff, act);
        st4(out + ((img * hp + oy + pad) * wp + ox + pad) * ldo + c0, lerp_blend4(v00, v01, v10, v11, lx.f, ly.f));
    }
}

// x4 in both directions (the DeepLabV3+ decoder's up-sampling of the ASPP output): a thread owns one INPUT pixel's 4 x 4 block of
// outputs and one 4-channel vector.  Those sixteen outputs interpolate between the 3 x 3 inputs around it, which the thread loads
// (and activates) once -- 9 loads per 16 outputs where the kernel above does 64 -- and every output is formed by the same
// expression from the same operands: bit-identical.
__global__ void __launch_bounds__(256) bilinear_fwd_x4_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                             int act, int ldx, float* __restrict__ out, int ldo, int n, int h, int w, int cv, int pad) {
    const long long total = (long long)n * h * w * cv;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c0 = (int)(i % cv) * 4;
    long long r = i / cv;
    const int bx = (int)(r % w); r /= w;
    const int by = (int)(r % h);
    const long long img = r / h;
    const bool aff = scale != nullptr;
    float4 s = f4(0.f), t = f4(0.f);
    if (aff) { s = ld4(scale + c0); t = ld4(shift + c0); }
    const float* base = x + img * h * w * ldx + c0;
    float4 v[3][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        int yy = by - 1 + dy;
        yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            int xx = bx - 1 + dx;
            xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
            v[dy][dx] = view_apply4(ld4(base + ((long long)yy * w + xx) * ldx), s, t, aff, act);
        }
    }
    const int ho = h * 4, wo = w * 4;
    const int hp = ho + 2 * pad, wp = wo + 2 * pad;
    Lerp lx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) lx[j] = lerp_of(bx * 4 + j, w, 0.25f);
#pragma unroll
    for (int jy = 0; jy < 4; ++jy) {
        const int oy = by * 4 + jy;
        const Lerp ly = lerp_of(oy, h, 0.25f);
        // rows i0, i1 of the source are rows (i - (by - 1)) of the cache; a clamped border row was loaded under its clamped index
        const int r0 = ly.i0 - (by - 1), r1 = ly.i1 - (by - 1);
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const int q0 = lx[jx].i0 - (bx - 1), q1 = lx[jx].i1 - (bx - 1);
            float4 v00, v01, v10, v11;
            // (compile-time indexed selects: the cache stays in registers)
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    if (a == r0 && b == q0) v00 = v[a][b];
                    if (a == r0 && b == q1) v01 = v[a][b];
                    if (a == r1 && b == q0) v10 = v[a][b];
                    if (a == r1 && b == q1) v11 = v[a][b];
                }
            st4(out + ((img * hp + oy + pad) * wp + bx * 4 + jx + pad) * ldo + c0, lerp_blend4(v00, v01, v10, v11, lx[jx].f, ly.f));
        }
    }
}

// gather form of the transposed resize: each input pixel sums the outputs that referenced it (deterministic)
__global__ void bilinear_bwd_kernel(const float* __restrict__ g, int ldg, float* __restrict__ dx, int ldx, int n, int h, int w, int cv,
                                    int fy, int fx, int accumulate) {
    const int ho = h * fy, wo = w * fx;
    const long long total = (long long)n * h * w * cv;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cv) * 4;
        long long r = i / cv;
        const int ix = (int)(r % w); r /= w;
        const int iy = (int)(r % h);
        const long long img = r / h;
        const LerpWindow win = lerp_window(iy, ix, h, w, fy, fx);
        float4 acc = f4(0.f);
        for (int oy = win.oy0; oy <= win.oy1; ++oy) {
            const float wy = lerp_weight(oy, iy, h, ify);
            if (wy == 0.f) continue;
            for (int ox = win.ox0; ox <= win.ox1; ++ox) {
                const float wx = lerp_weight(ox, ix, w, ifx);
                if (wx == 0.f) continue;
                axpy4(acc, wy * wx, ld4(g + ((img * ho + oy) * wo + ox) * ldg + c0));
            }
        }
        float* p = dx + ((img * h + iy) * w + ix) * ldx + c0;
        if (accumulate) add4(acc, ld4(p));
        st4(p, acc);
    }
}

// x4 in both directions (the gradient of the decoder's up-sampled ASPP output, 614,400 x 256 -> 38,400 x 256 at batch 32): a thread
// owns a 2 x 2 block of INPUT pixels and one 4-channel vector.  The four pixels' supports (8 x 8 outputs each) overlap: their union
// is 12 x 12 outputs, every one of which is loaded ONCE and added to the up to four pixels it belongs to -- 36 loads per input
// pixel where the gather kernel above does 64 behind two lerp_weight evaluations each; the weights of the 12 rows / columns are
// formed once per thread by the same lerp_weight (borders and clamping included).  Fixed summation order (rows, then columns).
__global__ void __launch_bounds__(256) bilinear_bwd_x4_kernel(const float* __restrict__ g, int ldg, float* __restrict__ dx, int ldx, int n, int h, int w,
                                                             int cv, int accumulate) {
    const int hb = (h + 1) >> 1, wb = (w + 1) >> 1, ho = h * 4, wo = w * 4;
    const long long total = (long long)n * hb * wb * cv;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c0 = (int)(i % cv) * 4;
    long long r = i / cv;
    const int bx = (int)(r % wb); r /= wb;
    const int by = (int)(r % hb);
    const long long img = r / hb;
    const int iy0 = 2 * by, ix0 = 2 * bx;
    const int oy0 = 4 * iy0 - 2, ox0 = 4 * ix0 - 2;          // first output row / column of the union window (may be < 0)
    float wy[12][2], wx[12][2];
#pragma unroll
    for (int k = 0; k < 12; ++k)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int oy = oy0 + k, ox = ox0 + k;
            wy[k][a] = (oy >= 0 && oy < ho && iy0 + a < h) ? lerp_weight(oy, iy0 + a, h, 0.25f) : 0.f;
            wx[k][a] = (ox >= 0 && ox < wo && ix0 + a < w) ? lerp_weight(ox, ix0 + a, w, 0.25f) : 0.f;
        }
    float4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f4(0.f);
    const float* base = g + img * ho * wo * (long long)ldg + c0;
#pragma unroll 2
    for (int ky = 0; ky < 12; ++ky) {
        const int oy = oy0 + ky;
        if (oy < 0 || oy >= ho) continue;
        const float* row = base + (long long)oy * wo * ldg;
        float4 v[12];
#pragma unroll
        for (int kx = 0; kx < 12; ++kx) {
            int ox = ox0 + kx;
            ox = ox < 0 ? 0 : (ox > wo - 1 ? wo - 1 : ox);      // (clamped columns carry weight 0)
            v[kx] = ld4(row + (long long)ox * ldg);
        }
#pragma unroll
        for (int kx = 0; kx < 12; ++kx)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) axpy4(acc[a][b], wy[ky][a] * wx[kx][b], v[kx]);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (iy0 + a < h && ix0 + b < w) {
                float* p = dx + ((img * h + iy0 + a) * w + ix0 + b) * (long long)ldx + c0;
                float4 o = acc[a][b];
                if (accumulate) add4(o, ld4(p));
                st4(p, o);
            }
        }
}

}  // namespace

extern "C" {

int ssdseg_gap_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, float* out, int n, int hw, int c) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(out != nullptr, 3);
    SSDSEG_ARG(n > 0, 4);
    SSDSEG_ARG(hw > 0, 5);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 6);
    return pixel_sum(ctx, in->x, c, in->scale, in->shift, in->act, out, c, n, hw, c, 1.f / (float)hw, 0,
                     4.0 * ((double)n * hw * c + (double)n * c));
}

int ssdseg_gap_bwd(ssdseg_ctx* ctx, const float* g, float* dx, int n, int hw, int c, int accumulate) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(g != nullptr, 2);
    SSDSEG_ARG(dx != nullptr, 3);
    SSDSEG_ARG(n > 0 && hw > 0, 4);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 6);
    const long long total = (long long)n * hw * (c / 4);
    SSDSEG_LAUNCH(ctx, 4.0 * n * hw * c * (accumulate ? 2 : 1), 0.0, gap_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, g, dx, n, hw, c / 4,
                  accumulate);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// the x4 kernels take an up-sampling by 4 in both directions unless SSDSEG_BILINEAR=gather asks for the general kernels (A/B runs,
// parity tests)
static bool x4_kernels(int fy, int fx) { return fy == 4 && fx == 4 && env_pick("SSDSEG_BILINEAR", {"gather"}) == 0; }

static int bilinear_fwd_impl(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, float* out, int ldo, int n, int h, int wdt, int c, int fy, int fx,
                             int pad) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= c && ldx % 4 == 0, 3);
    SSDSEG_ARG(out != nullptr, 4);
    SSDSEG_ARG(ldo >= c && ldo % 4 == 0, 5);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 6);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 9);
    SSDSEG_ARG(fy >= 1 && fx >= 1, 10);
    const long long total = (long long)n * h * fy * wdt * fx * (c / 4);
    const double cost = 4.0 * ((double)n * h * wdt * c + 4.0 * total);
    if (x4_kernels(fy, fx)) {
        const long long threads = (long long)n * h * wdt * (c / 4);
        SSDSEG_LAUNCH(ctx, cost, 0.0, bilinear_fwd_x4_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, in->x, in->scale, in->shift,
                      in->act, ldx, out, ldo, n, h, wdt, c / 4, pad);
        SSDSEG_LAUNCH_CHECK();
        return 0;
    }
    SSDSEG_LAUNCH(ctx, cost, 0.0, bilinear_fwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, in->x, in->scale, in->shift, in->act, ldx, out, ldo, n,
                  h, wdt, c / 4, fy, fx, pad);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_bilinear_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, float* out, int ldo, int n, int h, int wdt, int c, int fy,
                        int fx) {
    return bilinear_fwd_impl(ctx, in, ldx, out, ldo, n, h, wdt, c, fy, fx, 0);
}

// the same values written into the INTERIOR of a bordered tensor out[n][h*fy + 2][w*fx + 2][ldo] (the border is left alone): the
// up-sampled ASPP output lands directly in the zero-bordered input copy the decoder's 3x3 conv kernels read (ssdseg_conv3x3_fwd_saved_from)
int ssdseg_bilinear_fwd_padded(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, float* out, int ldo, int n, int h, int wdt, int c, int fy,
                               int fx) {
    return bilinear_fwd_impl(ctx, in, ldx, out, ldo, n, h, wdt, c, fy, fx, 1);
}

int ssdseg_bilinear_bwd(ssdseg_ctx* ctx, const float* g, int ldg, float* dx, int ldx, int n, int h, int wdt, int c, int fy, int fx,
                        int accumulate) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(g != nullptr, 2);
    SSDSEG_ARG(ldg >= c && ldg % 4 == 0, 3);
    SSDSEG_ARG(dx != nullptr, 4);
    SSDSEG_ARG(ldx >= c && ldx % 4 == 0, 5);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 6);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 9);
    SSDSEG_ARG(fy >= 1 && fx >= 1, 10);
    if (h == 1 && wdt == 1)   // a 1x1 source feeds every output pixel with weight 1 (the ASPP pooling branch): a plain pixel sum
        return pixel_sum(ctx, g, ldg, nullptr, nullptr, SSDSEG_ACT_NONE, dx, ldx, n, fy * fx, c, 1.f, accumulate,
                         4.0 * ((double)n * c * (1 + fy * fx)));
    const double cost = 4.0 * ((double)n * h * wdt * c * (1 + fy * fx));
    if (x4_kernels(fy, fx)) {
        const long long threads = (long long)n * ((h + 1) / 2) * ((wdt + 1) / 2) * (c / 4);
        SSDSEG_LAUNCH(ctx, cost, 0.0, bilinear_bwd_x4_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, g,
                      ldg, dx, ldx, n, h, wdt, c / 4, accumulate);
        SSDSEG_LAUNCH_CHECK();
        return 0;
    }
    const long long total = (long long)n * h * wdt * (c / 4);
    SSDSEG_LAUNCH(ctx, cost, 0.0, bilinear_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, g, ldg,
                  dx, ldx, n, h, wdt, c / 4, fy, fx, accumulate);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
