// Adam as Keras 2.13 applies it (NB03#cell14: tf.keras.optimizers.Adam(1e-4); semantics SURVEY.md App. B.10):
//   m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2);  p -= lr*sqrt(1 - b2^t)/(1 - b1^t) * m / (sqrt(v) + eps)
// One fused multi-tensor pass over the flat parameter bucket (HBM-bound: 4 streams read, 3 written).
// AdamW (ssdseg_adamw_step) is the same body with the decoupled decay p -= (lr lambda) p compiled in front of it; lambda comes
// from the run table (decay_runs.h), which also makes a block's float4s one contiguous chunk instead of a grid-stride comb.
// ssdseg_adamw_step_clipped (K20c) is the same kernel with g' = clampv((g * grad_scale) * s) compiled in (CLIP; grad_clip.h).
#include <math.h>

#include "common.h"
#include "decay_runs.h"
#include "grad_clip.h"

namespace {
template <bool DECAY, bool CLIP>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float alpha, float one_minus_b1, float one_minus_b2,
                                             float eps, float gscale, float lr, float lam, float s, float c) {
    float gk = g * gscale;
    if (CLIP) gk = clampv(gk * s, c);
    if (DECAY) p = decay_apply(p, lr, lam);
    m += (gk - m) * one_minus_b1;
    v += (gk * gk - v) * one_minus_b2;
    p -= alpha * m / (sqrtf(v) + eps);
}

// the float4 step of decay_walk (decay_runs.h)
template <bool CLIP>
struct AdamWalk {
    float* p; const float* g; float* m; float* v;
    float alpha, one_minus_b1, one_minus_b2, eps, gscale, lr, s, c;
    float4 pp, gg, mm, vv;
    __device__ __forceinline__ void load(size_t i) { pp = ld4(p + 4 * i); gg = ld4(g + 4 * i); mm = ld4(m + 4 * i); vv = ld4(v + 4 * i); }
    __device__ __forceinline__ void apply(const float lam[4]) {
        float* pe = &pp.x; float* ge = &gg.x; float* me = &mm.x; float* ve = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) adam_element<true, CLIP>(pe[k], ge[k], me[k], ve[k], alpha, one_minus_b1, one_minus_b2, eps, gscale, lr, lam[k], s, c);
    }
    __device__ __forceinline__ void store(size_t i) { st4(p + 4 * i, pp); st4(m + 4 * i, mm); st4(v + 4 * i, vv); }
};

template <bool DECAY, bool CLIP>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n4,
                            size_t n, float alpha, float one_minus_b1, float one_minus_b2, float eps, float gscale, float lr, DecayRuns runs,
                            GradClip clip) {
    const float s = CLIP ? clip_factor(clip) : 1.f, c = clip.value;
    if (!DECAY) {
        const size_t stride = (size_t)gridDim.x * blockDim.x;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            float4 pp = ld4(p + 4 * i), gg = ld4(g + 4 * i), mm = ld4(m + 4 * i), vv = ld4(v + 4 * i);
            float* pe = &pp.x; float* ge = &gg.x; float* me = &mm.x; float* ve = &vv.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) adam_element<false, CLIP>(pe[k], ge[k], me[k], ve[k], alpha, one_minus_b1, one_minus_b2, eps, gscale, lr, 0.f, s, c);
            st4(p + 4 * i, pp); st4(m + 4 * i, mm); st4(v + 4 * i, vv);
        }
    } else {
        AdamWalk<CLIP> w = {p, g, m, v, alpha, one_minus_b1, one_minus_b2, eps, gscale, lr, s, c, f4(0.f), f4(0.f), f4(0.f), f4(0.f)};
        decay_walk(runs, n4, w);
    }
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = (n4 << 2) + threadIdx.x;
        const float lam = DECAY ? decay_seek(runs, (long long)i).lam : 0.f;
        float pi = p[i], mi = m[i], vi = v[i];
        adam_element<DECAY, CLIP>(pi, g[i], mi, vi, alpha, one_minus_b1, one_minus_b2, eps, gscale, lr, lam, s, c);
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
}

// what the three entries share: the argument checks, reported under the entry's name, then the launch.  ssdseg_adam_step has no
// table (arguments 13 to 15) and only the clipped entry has clip_value, its 17th argument.
template <bool CLIP>
int adam_launch(const char* entry, ssdseg_ctx* ctx, float* params, const float* grads, float* m, float* v, size_t count, float lr, float beta1,
                float beta2, float eps, int step, float grad_scale, const long long* run_end, const float* run_decay, int nruns,
                const float* clip_scale, float clip_value) {
    SSDSEG_ARG_AS(entry, ctx != nullptr, 1);
    SSDSEG_ARG_AS(entry, params && grads && m && v, 2);
    SSDSEG_ARG_AS(entry, step >= 1, 11);
    SSDSEG_DECAY_ARGS(entry, run_end, run_decay, nruns, 13, 14, 15);
    if (CLIP) SSDSEG_ARG_AS(entry, clip_value > 0.f, 17);   // +inf: no clamp; fails for NaN
    if (count == 0) return 0;
    { int jrc = ssdseg_join(ctx); if (jrc) return jrc; }   // weight gradients may still be in flight on the side stream
    const double alpha = (double)lr * sqrt(1.0 - pow((double)beta2, step)) / (1.0 - pow((double)beta1, step));
    const size_t n4 = count / 4;
    const DecayRuns runs = {run_end, run_decay, nruns};
    const GradClip clip = {clip_scale, clip_value};
    if (nruns == 0)
        SSDSEG_LAUNCH_NAMED(ctx, CLIP ? "adam_clipped_kernel" : "adam_kernel", 28.0 * (double)count, 0.0, (adam_kernel<false, CLIP>),
                            dim3(optimizer_blocks(n4)), dim3(256), 0, params, grads, m, v, n4, count, (float)alpha, 1.f - beta1, 1.f - beta2, eps,
                            grad_scale, lr, runs, clip);
    else
        SSDSEG_LAUNCH_NAMED(ctx, CLIP ? "adamw_clipped_kernel" : "adamw_kernel", 28.0 * (double)count + 12.0 * nruns, 0.0,
                            (adam_kernel<true, CLIP>), dim3(decay_blocks(n4)), dim3(256), 0, params, grads, m, v, n4, count, (float)alpha,
                            1.f - beta1, 1.f - beta2, eps, grad_scale, lr, runs, clip);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int ssdseg_adam_step(ssdseg_ctx* ctx, float* params, const float* grads, float* m, float* v, size_t count, float lr,
                                float beta1, float beta2, float eps, int step, float grad_scale) {
    return adam_launch<false>(__func__, ctx, params, grads, m, v, count, lr, beta1, beta2, eps, step, grad_scale, nullptr, nullptr, 0, nullptr, 0.f);
}

extern "C" int ssdseg_adamw_step(ssdseg_ctx* ctx, float* params, const float* grads, float* m, float* v, size_t count, float lr,
                                 float beta1, float beta2, float eps, int step, float grad_scale, const long long* run_end,
                                 const float* run_decay, int nruns) {
    return adam_launch<false>(__func__, ctx, params, grads, m, v, count, lr, beta1, beta2, eps, step, grad_scale, run_end, run_decay, nruns,
                              nullptr, 0.f);
}

extern "C" int ssdseg_adamw_step_clipped(ssdseg_ctx* ctx, float* params, const float* grads, float* m, float* v, size_t count, float lr,
                                         float beta1, float beta2, float eps, int step, float grad_scale, const long long* run_end,
                                         const float* run_decay, int nruns, const float* clip_scale, float clip_value) {
    return adam_launch<true>(__func__, ctx, params, grads, m, v, count, lr, beta1, beta2, eps, step, grad_scale, run_end, run_decay, nruns,
                             clip_scale, clip_value);
}
