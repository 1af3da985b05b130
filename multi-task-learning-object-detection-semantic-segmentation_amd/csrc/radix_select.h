// What the two exact selections share (losses.hip: batch-global top-k of the mined confidence loss; mask_head.hip: per-image k-th
// largest pixel loss of the bootstrapped cross-entropy): the order-preserving 32-bit key of a float, and the MSB-first walk over
// the 256-bin histograms of four 8-bit passes.  All of it is integer work: the result does not depend on scheduling.
#pragma once
#include "common.h"

__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // larger float <=> larger unsigned key
}
// the float a key was made from
__device__ __forceinline__ float order_key_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// Every block re-derives the selection from the finished histograms of the earlier passes (256 ints each: cheaper than a
// one-block kernel between passes): prefix = the top 8*npass bits of the k-th largest key, krem = its rank inside that bucket.
// hist[p][b]: keys matching the prefix chosen by passes < p whose byte p (from the top) is b.  For a block of 256 threads; lh: 256 ints
// of LDS.
__device__ __forceinline__ void radix_select_prefix(const int (*__restrict__ hist)[256], int npass, int k, int* lh, unsigned* s_prefix,
                                                    int* s_krem) {
    const int t = threadIdx.x;
    if (t == 0) { *s_prefix = 0u; *s_krem = k; }
    for (int p = 0; p < npass; ++p) {
        __syncthreads();
        lh[t] = hist[p][t];
        __syncthreads();
        if (t == 0) {
            int krem = *s_krem, bin = 255;
            for (; bin > 0; --bin) {
                if (lh[bin] >= krem) break;
                krem -= lh[bin];
            }
            *s_prefix |= (unsigned)bin << (24 - 8 * p);
            *s_krem = krem;
        }
    }
    __syncthreads();
}
