// What resize.hip, mask_head.hip and heads.hip share: the half-pixel bilinear geometry (source rows / columns of an output, the
// four-corner blend, the output window of an input pixel), the 4-class softmax, the 256-thread block sum, and a host helper.
// Each expression is written here once: the kernels that claim bit-identity with one another (x4 / general resize, tile / gather
// mask-head backward) get it from the same text.  Units are built with -ffp-contract=fast: keep the written form of every
// product and sum.
#pragma once
#include "common.h"

// four host floats (class weights, box standard deviations) as a kernel argument
static inline float4 f4_of(const float* v) { return make_float4(v[0], v[1], v[2], v[3]); }

constexpr float KEPS = 1e-7f;  // tf.keras.backend.epsilon()

__device__ __forceinline__ void axpy4(float4& a, float s, float4 b) {
    a.x = fmaf(s, b.x, a.x); a.y = fmaf(s, b.y, a.y); a.z = fmaf(s, b.z, a.z); a.w = fmaf(s, b.w, a.w);
}

__device__ __forceinline__ float4 softmax4(float4 z) {
    const float m = fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w));
    float4 e = make_float4(expf(z.x - m), expf(z.y - m), expf(z.z - m), expf(z.w - m));
    const float inv = 1.f / (e.x + e.y + e.z + e.w);
    return make_float4(e.x * inv, e.y * inv, e.z * inv, e.w * inv);
}

// tf.image.resize(bilinear, half_pixel_centers=True): src = (dst + 0.5) * (in/out) - 0.5, clamped to [0, in-1]
struct Lerp {
    int i0, i1;
    float f;
};
__device__ __forceinline__ Lerp lerp_of(int dst, int in_size, float inv_factor) {
    float src = ((float)dst + 0.5f) * inv_factor - 0.5f;
    src = fminf(fmaxf(src, 0.f), (float)(in_size - 1));
    Lerp l;
    l.i0 = (int)floorf(src);
    l.i1 = l.i0 + 1 < in_size ? l.i0 + 1 : in_size - 1;
    l.f = src - (float)l.i0;
    return l;
}
// weight with which input index `i` contributes to output index `dst`
__device__ __forceinline__ float lerp_weight(int dst, int i, int in_size, float inv_factor) {
    const Lerp l = lerp_of(dst, in_size, inv_factor);
    return (l.i0 == i ? 1.f - l.f : 0.f) + (l.i1 == i ? l.f : 0.f);
}

// the output between the four inputs (rows i0 / i1, columns i0 / i1) around it: along x in both rows, then along y
__device__ __forceinline__ float4 lerp_blend4(float4 v00, float4 v01, float4 v10, float4 v11, float fx, float fy) {
    float4 top, bot, o;
    top.x = v00.x + (v01.x - v00.x) * fx; top.y = v00.y + (v01.y - v00.y) * fx; top.z = v00.z + (v01.z - v00.z) * fx; top.w = v00.w + (v01.w - v00.w) * fx;
    bot.x = v10.x + (v11.x - v10.x) * fx; bot.y = v10.y + (v11.y - v10.y) * fx; bot.z = v10.z + (v11.z - v10.z) * fx; bot.w = v10.w + (v11.w - v10.w) * fx;
    o.x = top.x + (bot.x - top.x) * fy; o.y = top.y + (bot.y - top.y) * fy; o.z = top.z + (bot.z - top.z) * fy; o.w = top.w + (bot.w - top.w) * fy;
    return o;
}

// The outputs that can draw from input pixel (iy, ix) of an h x w image up-sampled by (fy, fx): rows [oy0, oy1], columns [ox0, ox1].
// Input index i takes weight from the output indices whose source coordinate (o + 0.5) / f - 0.5 lies in (i - 1, i + 1):
// o in ((i - 0.5) * f - 0.5, (i + 1.5) * f - 0.5), i.e. [i*f - f/2, i*f + f + f/2 - 1]; a border pixel also takes every output
// clamped onto it.  The candidate range runs a little wider -- [i*f - f/2 - f, i*f + f + f/2 + 1], at most lerp_window_max(f)
// indices -- and callers skip the zero weights (lerp_weight) before touching memory.
struct LerpWindow {
    int oy0, oy1, ox0, ox1;
};
constexpr int lerp_window_max(int f) { return 3 * f + 2; }
__device__ __forceinline__ LerpWindow lerp_window(int iy, int ix, int h, int w, int fy, int fx) {
    const int ho = h * fy, wo = w * fx;
    LerpWindow r;
    r.oy0 = (iy == 0) ? 0 : (iy * fy - fy / 2 - fy); r.oy1 = (iy == h - 1) ? ho - 1 : (iy * fy + fy + fy / 2 + 1);
    r.ox0 = (ix == 0) ? 0 : (ix * fx - fx / 2 - fx); r.ox1 = (ix == w - 1) ? wo - 1 : (ix * fx + fx + fx / 2 + 1);
    r.oy0 = r.oy0 < 0 ? 0 : r.oy0; r.ox0 = r.ox0 < 0 ? 0 : r.ox0;
    r.oy1 = r.oy1 > ho - 1 ? ho - 1 : r.oy1; r.ox1 = r.ox1 > wo - 1 ? wo - 1 : r.ox1;
    return r;
}

// Sum over the 256 threads of a block of N values per thread, through red[N][256] in LDS: strides 128, 64, ..., 1, thread t adds
// element t + s -- one fixed order per value, however many are folded per pass.  The sums are red[k][0] after the call (the last
// barrier is inside).  A caller that reuses `red` puts a barrier in front of the next call.
template <typename T, int N>
__device__ __forceinline__ void block_sum256(const T (&v)[N], T (&red)[N][256]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][t] = v[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < N; ++k) red[k][t] += red[k][t + s];
        __syncthreads();
    }
}
