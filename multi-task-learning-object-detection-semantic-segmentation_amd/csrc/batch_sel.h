// How a block of the input-pipeline kernels (inputs.hip, crop.hip, mosaic.hip) learns which source sample it reads and whether it mirrors it,
// and the host code that goes with that.  blockIdx.y is the sample within one launch, n0 the launch's first output sample; a
// selection `sel` answers for output sample n0 + n with
//   sel.source(n0, n)     its source sample (64-bit: sample * h * w * 3 passes 2^32 at 4,661 samples of 480x640)
//   sel.mirrored(n0, n)   its flip flag
// and says in `chunk` how many samples one launch may cover.  No floating-point arithmetic in here: crop.hip and mosaic.hip are built
// with another -ffp-contract than inputs.hip (their sampling arithmetic is in crop_sample.h).
#pragma once
#include <cmath>

#include "common.h"

constexpr int GRID_Y_MAX = 65535;

// a plain batch: output n from source n, the flags in a device array (or NULL: none).  Nothing per sample travels with the
// launch, so one launch takes as many samples as gridDim.y allows.
struct plain_sel {
    static constexpr int chunk = GRID_Y_MAX;
    const uint8_t* flip;
    __device__ __forceinline__ long long source(int n0, int n) const { return n0 + n; }
    __device__ __forceinline__ bool mirrored(int n0, int n) const { return flip != nullptr && flip[n0 + n] != 0; }
};

// a gathered batch: HOST lists of source samples and flags, `chunk` samples per launch BY VALUE in the kernel arguments -- no
// host -> device copy of its own, nothing the caller could overwrite while it is in flight, no synchronisation (wave-uniform
// reads of the argument block)
struct gather_sel {
    static constexpr int chunk = 64;
    int32_t index[chunk];            // source sample of output sample n0 + n
    unsigned long long flip;         // bit n: its flag
    __device__ __forceinline__ long long source(int, int n) const { return index[n]; }
    __device__ __forceinline__ bool mirrored(int, int n) const { return ((flip >> n) & 1ull) != 0; }
};

// samples [n0, n0 + count) of the host lists as one kernel-argument block; index_host NULL: n -> n, flip_host NULL: no flags
static inline gather_sel make_sel(const int32_t* index_host, const uint8_t* flip_host, int n0, int count) {
    gather_sel sel;
    memset(&sel, 0, sizeof(sel));
    for (int i = 0; i < count; ++i) {
        sel.index[i] = index_host != nullptr ? index_host[n0 + i] : n0 + i;
        if (flip_host != nullptr && flip_host[n0 + i] != 0) sel.flip |= 1ull << i;
    }
    return sel;
}

// every source sample of a batch of b exists; index_host NULL: n -> n
static inline bool indices_in_source(const int32_t* index_host, int b, int n_src) {
    if (index_host == nullptr) return b <= n_src;
    for (int i = 0; i < b; ++i)
        if (index_host[i] < 0 || index_host[i] >= n_src) return false;
    return true;
}

// the four colour draws (hue, saturation, contrast, brightness)
static inline bool draws_finite(const float* d4) {
    return std::isfinite(d4[0]) && std::isfinite(d4[1]) && std::isfinite(d4[2]) && std::isfinite(d4[3]);
}

// status of the launch just queued, for code whose __func__ (a lambda's, a template's) would say nothing: `what` is the kernel
static inline int launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? ssdseg_hip_fail(e, what) : 0;
}

// launch(n0, count) for a batch of b in launches of at most `chunk` samples; stops at, and returns, the first non-zero status
template <typename F>
int for_each_chunk(int b, int chunk, F launch) {
    for (int n0 = 0; n0 < b; n0 += chunk) {
        const int rc = launch(n0, b - n0 < chunk ? b - n0 : chunk);
        if (rc) return rc;
    }
    return 0;
}

// launches the <true> (Vec) or <false> (Scalar) instantiation of one `template <bool VEC, ...>` kernel; the timing entry is
// `name` with that argument
template <auto Vec, auto Scalar, typename... Args>
int launch_vec(ssdseg_ctx* ctx, bool vec, const char* name, double bytes, dim3 grid, int threads, Args... args) {
    const char* kname = name;
    if (ctx->timing) {
        char buf[96];
        snprintf(buf, sizeof(buf), "%s<%s>", name, vec ? "true" : "false");
        kname = ssdseg_intern(buf);
    }
    if (vec) SSDSEG_LAUNCH_NAMED(ctx, kname, bytes, 0.0, Vec, grid, dim3(threads), 0, args...);
    else SSDSEG_LAUNCH_NAMED(ctx, kname, bytes, 0.0, Scalar, grid, dim3(threads), 0, args...);
    return launch_status(name);
}
