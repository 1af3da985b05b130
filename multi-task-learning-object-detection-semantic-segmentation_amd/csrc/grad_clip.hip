// Global-norm gradient clipping (tf.clip_by_global_norm, Keras 2.13's `global_clipnorm`) and the EMA of the weights (`use_ema`),
// include/ssdseg.h K20c.
//   ssdseg_grad_norm : out[0] = |grad_scale| sqrt(sum g^2),  out[1] = norm > clip_norm ? clip_norm / norm : 1
//   ssdseg_ema_update: ema += (p - ema)(1 - momentum)
// The norm is produced ON THE DEVICE and consumed there by the *_clipped step entries (sgd.hip, adam.hip) through a pointer: a
// factor that depends on this step's gradients never visits the host, so the step stays queued without a synchronisation.
// Squares and sums are fp64: the square of a float is exact in double (24 + 24 < 53 bits, exponent range 2 x 2^8 << 2^11), so a
// 1e-30 gradient neither underflows nor a 1e30 one overflows, and the sum's error is n 2^-53.
// Deterministic by construction: the partition depends on `count` only (decay_blocks / decay_chunk, as the step kernels), every
// thread folds its four float4 lanes' chains in one order, the block folds through LDS in one order (reduce_parts.h's shape: halve
// to 8, then serially), and a second one-block launch folds the blocks' partials in index order.  No atomics, no counter.
#include <float.h>
#include <math.h>

#include "common.h"
#include "decay_runs.h"

namespace {
constexpr int NT = 256;

// sum over the block of one double per thread, fixed order; valid in thread 0.  red: NT doubles of LDS
__device__ __forceinline__ double block_fold(double s, double* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int half = NT / 2; half >= 8; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int y = 0; y < 8; ++y) t += red[y];
    return t;
}

__device__ __forceinline__ void sq4(double (&acc)[4], float4 g) {
    acc[0] += (double)g.x * (double)g.x;
    acc[1] += (double)g.y * (double)g.y;
    acc[2] += (double)g.z * (double)g.z;
    acc[3] += (double)g.w * (double)g.w;
}

// partials[blockIdx.x] = sum of squares of this block's contiguous chunk (block 0: plus the scalar tail)
__global__ void __launch_bounds__(NT) grad_sumsq_kernel(const float* __restrict__ g, size_t n4, size_t n, double* __restrict__ partials) {
    __shared__ double red[NT];
    size_t first, last;
    decay_chunk(n4, &first, &last);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    size_t i = first + threadIdx.x;
    // two float4s in flight per thread: the kernel is one 4 B/element read and nothing else
    for (; i + NT < last; i += 2 * NT) {
        const float4 a = ld4(g + 4 * i), b = ld4(g + 4 * (i + NT));
        sq4(acc, a);
        sq4(acc, b);
    }
    if (i < last) sq4(acc, ld4(g + 4 * i));
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float t = g[(n4 << 2) + threadIdx.x];
        acc[0] += (double)t * (double)t;
    }
    const double s = block_fold((acc[0] + acc[1]) + (acc[2] + acc[3]), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one block: folds the partials in one fixed order (per thread, then through LDS); writes the norm and the clip factor
__global__ void __launch_bounds__(NT) grad_norm_finish_kernel(const double* __restrict__ partials, int nparts, float gscale, float clip_norm,
                                                              float* __restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    // eight independent loads per thread and trip (one trip: the grid cap is 2048 = 8 * NT): the block waits for memory once
    for (int base = threadIdx.x; base < nparts; base += 8 * NT) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base + u * NT < nparts ? partials[base + u * NT] : 0.0;
        s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    const double sum = block_fold(s, red);
    if (threadIdx.x == 0) {
        const double norm = fabs((double)gscale) * sqrt(sum);
        double factor = 1.0;
        // a NaN norm fails the comparison: the factor stays 1 and the non-finite gradients reach the weights as without clipping
        if (clip_norm > 0.f && clip_norm <= FLT_MAX && norm > (double)clip_norm) factor = (double)clip_norm / norm;
        out[0] = (float)norm;
        out[1] = (float)factor;
    }
}

__global__ void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n4, size_t n, float one_minus_momentum) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 ee = ld4(ema + 4 * i);
        const float4 pp = ld4(p + 4 * i);
        ee.x += (pp.x - ee.x) * one_minus_momentum;
        ee.y += (pp.y - ee.y) * one_minus_momentum;
        ee.z += (pp.z - ee.z) * one_minus_momentum;
        ee.w += (pp.w - ee.w) * one_minus_momentum;
        st4(ema + 4 * i, ee);
    }
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = (n4 << 2) + threadIdx.x;
        float e = ema[i];
        e += (p[i] - e) * one_minus_momentum;
        ema[i] = e;
    }
}
}  // namespace

extern "C" int ssdseg_grad_norm_parts(size_t count) { return (int)decay_blocks(count / 4); }

extern "C" int ssdseg_grad_norm(ssdseg_ctx* ctx, const float* grads, size_t count, float grad_scale, float clip_norm, double* partials,
                                float* out) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(grads != nullptr || count == 0, 2);
    SSDSEG_ARG(partials != nullptr || count == 0, 6);
    SSDSEG_ARG(out != nullptr, 7);
    { int jrc = ssdseg_join(ctx); if (jrc) return jrc; }   // weight gradients may still be in flight on the side stream
    const size_t n4 = count / 4;
    const int nparts = count ? (int)decay_blocks(n4) : 0;
    if (nparts)
        SSDSEG_LAUNCH(ctx, 4.0 * (double)count, 0.0, grad_sumsq_kernel, dim3(nparts), dim3(NT), 0, grads, n4, count, partials);
    SSDSEG_LAUNCH(ctx, 8.0 * nparts, 0.0, grad_norm_finish_kernel, dim3(1), dim3(NT), 0, partials, nparts, grad_scale, clip_norm, out);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

extern "C" int ssdseg_ema_update(ssdseg_ctx* ctx, float* ema, const float* params, size_t count, float momentum) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(ema != nullptr, 2);
    SSDSEG_ARG(params != nullptr, 3);
    SSDSEG_ARG(momentum >= 0.f && momentum <= 1.f, 5);
    if (count == 0) return 0;
    { int jrc = ssdseg_join(ctx); if (jrc) return jrc; }
    const size_t n4 = count / 4;
    SSDSEG_LAUNCH(ctx, 12.0 * (double)count, 0.0, ema_kernel, dim3(optimizer_blocks(n4)), dim3(256), 0, ema, params, n4, count, 1.f - momentum);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
