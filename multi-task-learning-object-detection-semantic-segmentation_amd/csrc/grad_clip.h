// The clip of the *_clipped optimizer entries (include/ssdseg.h, K20c): g' = clampv((g * grad_scale) * s, c).
//   s : *scale, the global-norm factor ssdseg_grad_norm left in device memory (NULL: 1) -- one block-uniform load per block
//   c : the clip value (+inf: no clamp)
#pragma once
#include "common.h"

struct GradClip {
    const float* scale;
    float value;
};

#ifdef __HIPCC__
__device__ __forceinline__ float clip_factor(const GradClip& clip) { return clip.scale ? *clip.scale : 1.f; }

// tf.clip_by_value: a NaN fails both comparisons and passes through (fminf(fmaxf(..)) would swallow it); identity at c = +inf
__device__ __forceinline__ float clampv(float x, float c) { return x < -c ? -c : (x > c ? c : x); }
#endif
