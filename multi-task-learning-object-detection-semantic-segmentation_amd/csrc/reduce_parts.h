// The partial-row reduction behind bn_finalize_kernel, bn_bwd_finalize_kernel (bn.hip), colsum_kernel and colsum_batch_kernel
// (colsum.hip): the device fold, the rule that picks the block shape from the table shape, and the one host dispatch over the shapes.
#pragma once
#include "common.h"
#include <type_traits>

// Partial-row reductions: blocks of RC channels x RP lanes along the partial rows (RC * RP == RTHREADS).  A table with many
// rows and few channels (BN partials of a 16..160-channel tensor: up to 2048 rows) would otherwise run on c/32 blocks with
// 64 dependent loads per thread; the narrow shape gives 4x the blocks and 4x fewer serial loads.
constexpr int RTHREADS = 256;   // small blocks: they have to find room next to the side stream's GEMM blocks

// Sums part[p][v][ch] over p for v < NV: RP lanes along p per channel, 4 independent fp64 chains per lane, then a fixed-
// order fold (deterministic).  Result valid for threadIdx.y == 0.  red: NV * RP * (RC + 1) doubles of LDS.
// CH: independent chains (= loads in flight) per lane and value: 4 for the two-value BatchNorm tables, 8 for the column sums of the
// weight-gradient slabs (tall tables read once: latency is all there is)
template <int NV, int RC, int CH = 4>
__device__ __forceinline__ void reduce_parts(const float* __restrict__ part, int nparts, int c, int ch, double (&tot)[NV], double* red,
                                             const int tx = threadIdx.x, const int ty = threadIdx.y) {
    constexpr int RP = RTHREADS / RC;
    double acc[NV][CH];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int u = 0; u < CH; ++u) acc[v][u] = 0.0;
    if (ch < c) {
        int p = ty;
        for (; p + (CH - 1) * RP < nparts; p += CH * RP) {
            float f[NV][CH];
#pragma unroll
            for (int u = 0; u < CH; ++u)
#pragma unroll
                for (int v = 0; v < NV; ++v) f[v][u] = part[((long long)(p + u * RP) * NV + v) * c + ch];
#pragma unroll
            for (int u = 0; u < CH; ++u)
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v][u] += (double)f[v][u];
        }
        for (; p < nparts; p += RP) {
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v][0] += (double)part[((long long)p * NV + v) * c + ch];
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double s = 0.0;
        if (CH == 4) s = (acc[v][0] + acc[v][1]) + (acc[v][2] + acc[v][3]);
        else {
#pragma unroll
            for (int u = 0; u < CH; u += 4) s += (acc[v][u] + acc[v][u + 1]) + (acc[v][u + 2] + acc[v][u + 3]);
        }
        red[(v * RP + ty) * (RC + 1) + tx] = s;
    }
    __syncthreads();
    // fold RP -> 8 lanes in parallel, then serially (fixed order either way)
    for (int half = RP / 2; half >= 8; half >>= 1) {
        if ((int)ty < half) {
#pragma unroll
            for (int v = 0; v < NV; ++v)
                red[(v * RP + ty) * (RC + 1) + tx] += red[(v * RP + ty + half) * (RC + 1) + tx];
        }
        __syncthreads();
    }
    if (ty == 0) {
        constexpr int LAST = RP < 8 ? RP : 8;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double s = 0.0;
            for (int y = 0; y < LAST; ++y) s += red[(v * RP + y) * (RC + 1) + tx];
            tot[v] = s;
        }
    }
}

// channels per block for a table of nparts rows
// (narrow blocks read 32-byte row segments, so they are only worth it while the table is too narrow to fill the chip)
inline int reduce_rc(int nparts, long long len) {
    if (nparts < 32) return 32;
    return (nparts >= 256 && len < 2048) ? 2 : 8;
}

// the one place that turns a run-time block shape into a template argument: f(std::integral_constant<int, RC>()) for rc in {2, 8, 32}
template <class F>
inline void for_rc(int rc, F f) {
    if (rc == 2) f(std::integral_constant<int, 2>());
    else if (rc == 8) f(std::integral_constant<int, 8>());
    else f(std::integral_constant<int, 32>());
}
