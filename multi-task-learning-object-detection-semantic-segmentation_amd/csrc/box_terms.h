// Per-anchor pieces of the box regression losses and the block reduction of the per-anchor passes, shared by losses.hip (smooth-L1
// fused with a confidence loss) and loc_iou.hip (IoU-family loss with the same smooth-L1 next to it): the same bits in both.
#pragma once
#include "common.h"

template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* red) {
    // deterministic tree over 256 threads; result in v[] of thread 0
    for (int k = 0; k < NV; ++k) {
        __syncthreads();
        red[threadIdx.x] = v[k];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        v[k] = red[0];
    }
}

// 1 for an anchor that carries a box target (localization_loss's own non-background test, losses.py:23-24)
__device__ __forceinline__ float has_box(float4 yb) { return (fabsf(yb.x) + fabsf(yb.y) + fabsf(yb.z) + fabsf(yb.w)) > 0.f ? 1.f : 0.f; }

// smooth-L1 of the four offset errors of one anchor (losses.py:30-40).  anchor_terms (losses.hip) keeps these lines in its own
// body: routed through this function its kernels compile to a different schedule, and their device code is to stay as it is.
__device__ __forceinline__ float sl1_sum(float4 yb, float4 pb) {
    const float e[4] = {yb.x - pb.x, yb.y - pb.y, yb.z - pb.z, yb.w - pb.w};
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float a = fabsf(e[k]);
        s += a < 1.f ? e[k] * e[k] * 0.5f : a - 0.5f;
    }
    return s;
}

// d smooth-L1 / d p_boxes of one anchor, times s (shared by every gradient pass: the same bits)
__device__ __forceinline__ float4 sl1_grad(float s, float4 ybx, float4 pbx) {
    const float e[4] = {ybx.x - pbx.x, ybx.y - pbx.y, ybx.z - pbx.z, ybx.w - pbx.w};
    float d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ab = fabsf(e[k]);
        d[k] = s * (ab < 1.f ? -e[k] : (e[k] > 0.f ? -1.f : (e[k] < 0.f ? 1.f : 0.f)));
    }
    return make_float4(d[0], d[1], d[2], d[3]);
}
