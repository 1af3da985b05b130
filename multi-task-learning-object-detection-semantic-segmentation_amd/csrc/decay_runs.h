// Weight-decay run table of the optimizer kernels (include/ssdseg.h, K20b): which lambda an element of the flat bucket takes.
//   end[r] : exclusive end offset of run r, in elements (run r covers [end[r-1], end[r]), run 0 starts at 0)
//   lam[r] : its decay coefficient;  elements at or beyond end[n-1] -- all of them when n == 0 -- take 0
// No per-element stream: a block owns a CONTIGUOUS chunk of the bucket (decay_chunk), finds the run of the chunk's first element
// with one bounded binary search on block-uniform values (scalar loads), and every thread then walks a cursor forward from
// there -- its elements only ascend.  The cursor keeps the current run's end and lambda in registers, so an iteration inside a
// run (the common case: a run is a whole tensor or several) reads nothing from the table.  The seek is a chain of dependent
// loads at the head of every block, so the kernels request their first float4s before it and let it run under them.
// Safety does not depend on the table's contents: every table index is in [0, n) (seek: lo <= mid < hi <= n; advance: r stops at
// n, where the end is LLONG_MAX), and the table never enters an address of p / g / m / v.  A table whose ends do not ascend gives
// each element the lambda of SOME run or 0, nothing worse.
#pragma once
#include <limits.h>

#include "common.h"

#ifdef __HIPCC__
struct DecayRuns {
    const long long* end;
    const float* lam;
    int n;
};

struct DecayCursor {
    int r;           // current run, n when beyond the table
    long long end;   // its end; LLONG_MAX beyond the table
    float lam;       // its lambda; 0 beyond the table
};

__device__ __forceinline__ void decay_load(const DecayRuns& t, DecayCursor& c) {
    if (c.r < t.n) {
        c.end = t.end[c.r];
        c.lam = t.lam[c.r];
    } else {
        c.end = LLONG_MAX;
        c.lam = 0.f;
    }
}

// the first run whose end lies beyond element e (at most ceil(log2(n + 1)) probes)
__device__ __forceinline__ DecayCursor decay_seek(const DecayRuns& t, long long e) {
    int lo = 0, hi = t.n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.end[mid] <= e) lo = mid + 1; else hi = mid;
    }
    DecayCursor c;
    c.r = lo;
    decay_load(t, c);
    return c;
}

// move the cursor to the run of element e, e no smaller than at the previous call
__device__ __forceinline__ void decay_advance(const DecayRuns& t, DecayCursor& c, long long e) {
    while (c.end <= e) {     // r < n here: beyond the table the end is LLONG_MAX
        ++c.r;
        decay_load(t, c);
    }
}

// lambdas of the four elements e .. e + 3 of one float4; leaves the cursor on the run of e
__device__ __forceinline__ void decay_lambda4(const DecayRuns& t, DecayCursor& c, long long e, float lam[4]) {
    decay_advance(t, c, e);
    lam[0] = lam[1] = lam[2] = lam[3] = c.lam;
    if (c.end < e + 4) {     // a boundary inside the float4 (ShuffleNetV2's 58- / 122-channel vectors end at offsets = 2 mod 4)
        DecayCursor k = c;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            decay_advance(t, k, e + j);
            lam[j] = k.lam;
        }
    }
}

// p1 = p - (lr lambda) p, lrlam = lr * lambda rounded once; lambda == 0 leaves p as it is, bit for bit (also -0 and NaN payloads)
__device__ __forceinline__ float decay_apply(float p, float lr, float lam) {
    const float lrlam = lr * lam;
    return lam != 0.f ? p - lrlam * p : p;
}

// float4 range [*first, *last) of this block: contiguous chunks of ceil(n4 / gridDim.x) float4s, rounded up to whole trips of
// the block (every block but the last one with work runs full trips, and chunks start on 4 KiB of each stream; the last blocks
// of a capped grid may then be left without work)
__device__ __forceinline__ void decay_chunk(size_t n4, size_t* first, size_t* last) {
    size_t chunk = (n4 + gridDim.x - 1) / gridDim.x;
    chunk = (chunk + blockDim.x - 1) / blockDim.x * blockDim.x;
    const size_t a = (size_t)blockIdx.x * chunk;
    const size_t b = a + chunk;
    *first = a < n4 ? a : n4;
    *last = b < n4 ? b : n4;
}

// One block's walk over its chunk.  W is the kernel's float4 step: it keeps a float4 per stream in registers and has load(i),
// apply(lam[4]) and store(i), i a float4 index.
template <class W>
__device__ __forceinline__ void decay_walk(const DecayRuns& runs, size_t n4, W& w) {
    size_t first, last;
    decay_chunk(n4, &first, &last);
    size_t i = first + threadIdx.x;
    // the first float4s are requested BEFORE the seek: its dependent scalar loads then run under loads the block waits for anyway
    if (i < last) w.load(i);
    DecayCursor cur = decay_seek(runs, (long long)(first << 2));
    while (i < last) {
        float lam[4];
        decay_lambda4(runs, cur, (long long)(i << 2), lam);
        w.apply(lam);
        w.store(i);
        i += blockDim.x;
        if (i < last) w.load(i);
    }
}
#endif

// host side: the run-table argument checks shared by the entries (argument numbers of run_end, run_decay, nruns), reported under
// the name `entry`
#define SSDSEG_DECAY_ARGS(entry, run_end, run_decay, nruns, a_end, a_decay, a_n)  \
    do {                                                                           \
        SSDSEG_ARG_AS(entry, (nruns) >= 0, a_n);                                   \
        SSDSEG_ARG_AS(entry, (nruns) == 0 || (run_end) != nullptr, a_end);         \
        SSDSEG_ARG_AS(entry, (nruns) == 0 || (run_decay) != nullptr, a_decay);     \
        SSDSEG_ARG_AS(entry, (nruns) <= SSDSEG_DECAY_RUNS_MAX, a_n);               \
    } while (0)

// grid of a grid-stride optimizer kernel: a thread per float4, at most 2048 blocks of 256 (csrc/adam.hip)
static inline unsigned optimizer_blocks(size_t n4) {
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// grid of a chunked kernel (decay_chunk): the same cap, less the blocks that the rounding to whole trips would leave without work.
// Whatever the grid, decay_chunk's chunks cover [0, n4): chunk >= n4 / gridDim.x.
static inline unsigned decay_blocks(size_t n4) {
    const size_t blocks = optimizer_blocks(n4);
    const size_t chunk = ((n4 + blocks - 1) / blocks + 255) / 256 * 256;
    return chunk ? (unsigned)((n4 + chunk - 1) / chunk) : 1u;
}
