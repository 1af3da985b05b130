// SGD as Keras 2.13 applies it (tf.keras.optimizers.SGD with its decoupled `weight_decay`), g' = g * grad_scale:
//   p1 = p - (lr lambda) p                                   lambda from the run table (decay_runs.h)
//   momentum == 0:  p = p1 - lr g'                           12 B per element, the velocity is not touched
//   momentum  > 0:  v = momentum v - lr g';  p = p1 + v      20 B per element
//        nesterov:  v likewise;  p = p1 + (momentum v - lr g')
// The recipe of the SSD and DeepLabV3+ papers (momentum 0.9, L2 decay on the convolution kernels, stepped / poly rate).
// One fused pass over the flat parameter bucket, as csrc/adam.hip: float4 body, scalar tail, a block per contiguous chunk.
// ssdseg_sgd_step_clipped (K20c) is the same kernel with g' = clampv((g * grad_scale) * s) compiled in (CLIP; grad_clip.h).
#include "common.h"
#include "decay_runs.h"
#include "grad_clip.h"

namespace {
enum { SGD_PLAIN = 0, SGD_MOMENTUM = 1, SGD_NESTEROV = 2 };

template <int MODE, bool CLIP>
__device__ __forceinline__ void sgd_element(float& p, float g, float& v, float lr, float mu, float gscale, float lam, float s, float c) {
    float gk = g * gscale;
    if (CLIP) gk = clampv(gk * s, c);
    const float p1 = decay_apply(p, lr, lam);
    if (MODE == SGD_PLAIN) {
        p = p1 - lr * gk;
    } else {
        v = mu * v - lr * gk;
        p = MODE == SGD_NESTEROV ? p1 + (mu * v - lr * gk) : p1 + v;
    }
}

// the float4 step of decay_walk (decay_runs.h)
template <int MODE, bool CLIP>
struct SgdWalk {
    float* p; const float* g; float* v;
    float lr, mu, gscale, s, c;
    float4 pp, gg, vv;
    __device__ __forceinline__ void load(size_t i) { pp = ld4(p + 4 * i); gg = ld4(g + 4 * i); if (MODE != SGD_PLAIN) vv = ld4(v + 4 * i); }
    __device__ __forceinline__ void apply(const float lam[4]) {
        float* pe = &pp.x; float* ge = &gg.x; float* ve = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) sgd_element<MODE, CLIP>(pe[k], ge[k], ve[k], lr, mu, gscale, lam[k], s, c);
    }
    __device__ __forceinline__ void store(size_t i) { st4(p + 4 * i, pp); if (MODE != SGD_PLAIN) st4(v + 4 * i, vv); }
};

template <int MODE, bool CLIP>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v, size_t n4, size_t n, float lr, float mu,
                           float gscale, DecayRuns runs, GradClip clip) {
    const float s = CLIP ? clip_factor(clip) : 1.f, c = clip.value;
    SgdWalk<MODE, CLIP> w = {p, g, v, lr, mu, gscale, s, c, f4(0.f), f4(0.f), f4(0.f)};
    decay_walk(runs, n4, w);
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = (n4 << 2) + threadIdx.x;
        const float lam = decay_seek(runs, (long long)i).lam;
        float pi = p[i], vi = MODE != SGD_PLAIN ? v[i] : 0.f;
        sgd_element<MODE, CLIP>(pi, g[i], vi, lr, mu, gscale, lam, s, c);
        p[i] = pi;
        if (MODE != SGD_PLAIN) v[i] = vi;
    }
}
// what both entries share: the argument checks, reported under the entry's name, then the launch.  clip_value is the 14th
// argument of the clipped entry.
template <bool CLIP>
int sgd_launch(const char* entry, ssdseg_ctx* ctx, float* params, const float* grads, float* velocity, size_t count, float lr, float momentum,
               int nesterov, float grad_scale, const long long* run_end, const float* run_decay, int nruns, const float* clip_scale,
               float clip_value) {
    SSDSEG_ARG_AS(entry, ctx != nullptr, 1);
    SSDSEG_ARG_AS(entry, params != nullptr, 2);
    SSDSEG_ARG_AS(entry, grads != nullptr, 3);
    SSDSEG_ARG_AS(entry, momentum >= 0.f && momentum < 1.f, 7);
    SSDSEG_ARG_AS(entry, velocity != nullptr || momentum == 0.f, 4);
    SSDSEG_DECAY_ARGS(entry, run_end, run_decay, nruns, 10, 11, 12);
    if (CLIP) SSDSEG_ARG_AS(entry, clip_value > 0.f, 14);   // +inf: no clamp; fails for NaN
    if (count == 0) return 0;
    { int jrc = ssdseg_join(ctx); if (jrc) return jrc; }   // weight gradients may still be in flight on the side stream
    const size_t n4 = count / 4;
    const unsigned blocks = decay_blocks(n4);
    const DecayRuns runs = {run_end, run_decay, nruns};
    const GradClip clip = {clip_scale, clip_value};
    const double bytes = (momentum > 0.f ? 20.0 : 12.0) * (double)count + 12.0 * nruns;
    if (momentum == 0.f)
        SSDSEG_LAUNCH_NAMED(ctx, CLIP ? "sgd_clipped_kernel" : "sgd_kernel", bytes, 0.0, (sgd_kernel<SGD_PLAIN, CLIP>), dim3(blocks), dim3(256), 0,
                            params, grads, velocity, n4, count, lr, momentum, grad_scale, runs, clip);
    else if (!nesterov)
        SSDSEG_LAUNCH_NAMED(ctx, CLIP ? "sgd_momentum_clipped_kernel" : "sgd_momentum_kernel", bytes, 0.0, (sgd_kernel<SGD_MOMENTUM, CLIP>),
                            dim3(blocks), dim3(256), 0, params, grads, velocity, n4, count, lr, momentum, grad_scale, runs, clip);
    else
        SSDSEG_LAUNCH_NAMED(ctx, CLIP ? "sgd_nesterov_clipped_kernel" : "sgd_nesterov_kernel", bytes, 0.0, (sgd_kernel<SGD_NESTEROV, CLIP>),
                            dim3(blocks), dim3(256), 0, params, grads, velocity, n4, count, lr, momentum, grad_scale, runs, clip);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int ssdseg_sgd_step(ssdseg_ctx* ctx, float* params, const float* grads, float* velocity, size_t count, float lr, float momentum,
                               int nesterov, float grad_scale, const long long* run_end, const float* run_decay, int nruns) {
    return sgd_launch<false>(__func__, ctx, params, grads, velocity, count, lr, momentum, nesterov, grad_scale, run_end, run_decay, nruns,
                             nullptr, 0.f);
}

extern "C" int ssdseg_sgd_step_clipped(ssdseg_ctx* ctx, float* params, const float* grads, float* velocity, size_t count, float lr,
                                       float momentum, int nesterov, float grad_scale, const long long* run_end, const float* run_decay,
                                       int nruns, const float* clip_scale, float clip_value) {
    return sgd_launch<true>(__func__, ctx, params, grads, velocity, count, lr, momentum, nesterov, grad_scale, run_end, run_decay, nruns,
                            clip_scale, clip_value);
}
