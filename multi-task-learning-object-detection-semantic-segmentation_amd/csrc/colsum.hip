// Column sums of the partial slabs that the weight-gradient kernels write (gemm.hip, pw_wgrad.hip, conv3.hip, dwconv.hip, stem.hip):
// out[l] = sum over the nparts rows of part[p][l], two-level with a fixed summation order (reduce_parts.h).
//
// Deferred column sums: nothing reads a weight gradient before the optimizer (or the all-reduce in front of it), so the ~80 column
// sums that fold the partial slabs of the weight-gradient kernels need not be ~80 launches scattered over the backward pass: while
// deferral is on, the slabs live in a persistent arena (ssdseg_partials), ssdseg_colsum only records (slab table, destination), and
// the first ssdseg_join afterwards -- the engine joins the side stream at the end of backward() -- folds them all with one launch.
#include "reduce_parts.h"
#include <vector>

namespace {

// out[l] = sum_p part[p][l]
template <int RC>
__global__ void __launch_bounds__(RTHREADS) colsum_kernel(const float* __restrict__ part, int nparts, int len, float* __restrict__ out) {
    __shared__ double red[(RTHREADS / RC) * (RC + 1)];
    const int l = blockIdx.x * RC + threadIdx.x;
    double tot[1] = {0.0};
    reduce_parts<1, RC, 8>(part, nparts, len, l, tot, red);
    if (threadIdx.y == 0 && l < len) out[l] = (float)tot[0];
}

// Every weight-gradient slab table of a backward pass in ONE launch.  Block b belongs to the entry whose block range contains it
// and does there exactly what a colsum_kernel<rc> block does (same lanes per column, same chains, same fold), so a gradient is the
// same bits whether its column sum was launched on its own or rides in the batch.
struct ColsumEntry {
    const float* part;
    float* out;
    int nparts, len, rc, block_begin;
};

// block lb of entry e as a colsum_kernel<RC> block: thread t of the flat block is (t % RC, t / RC) there
template <int RC>
__device__ __forceinline__ void colsum_block(const ColsumEntry& e, int lb, int t, double* red) {
    const int tx = t % RC, ty = t / RC, l = lb * RC + tx;
    double tot[1] = {0.0};
    reduce_parts<1, RC, 8>(e.part, e.nparts, e.len, l, tot, red, tx, ty);
    if (ty == 0 && l < e.len) e.out[l] = (float)tot[0];
}

__global__ void __launch_bounds__(RTHREADS) colsum_batch_kernel(const ColsumEntry* __restrict__ table, int n) {
    __shared__ double red[(RTHREADS / 2) * 3];       // the largest of the three shapes: (RTHREADS / RC) * (RC + 1) at RC = 2
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                 // last entry with block_begin <= blockIdx.x (block-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block_begin <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const ColsumEntry e = table[lo];
    const int lb = (int)blockIdx.x - e.block_begin, t = threadIdx.x;
    if (e.rc == 2) colsum_block<2>(e, lb, t, red);
    else if (e.rc == 8) colsum_block<8>(e, lb, t, red);
    else colsum_block<32>(e, lb, t, red);
}

}  // namespace

struct ssdseg_defer {
    struct Chunk { char* base; size_t cap, used; };
    bool on = false;
    int hold = 0;          // > 0: a composite entry point consumes the nested result at once -- no deferral (ssdseg_defer_hold)
    std::vector<Chunk> chunks;
    std::vector<ColsumEntry> pending, uploaded;
    ColsumEntry* d_table = nullptr;
    size_t d_cap = 0;
    double pending_bytes = 0.0;
};

static bool defer_owns(const ssdseg_defer* d, const void* p) {
    for (const auto& c : d->chunks)
        if ((const char*)p >= c.base && (const char*)p < c.base + c.cap) return true;
    return false;
}

// Arena size past which ssdseg_partials folds what is pending before it allocates more (SSDSEG_COLSUM_ARENA_MB, default 4 GiB: far
// above what one backward pass of the engine holds, so a pass never flushes early).  Bounds a loop of weight-gradient entry points
// called with deferral on and no join in between, whose slabs would otherwise stay allocated until the next join.
static size_t arena_cap() {
    const long long mb = env_int("SSDSEG_COLSUM_ARENA_MB", 0);
    return (size_t)(mb > 0 ? mb : 4096) << 20;
}

int ssdseg_partials(ssdseg_ctx* ctx, size_t bytes, void** out) {
    ssdseg_defer* d = ctx->defer;
    if (d == nullptr || !d->on || d->hold > 0) return ssdseg_workspace(ctx, bytes, out);
    bytes = (bytes + 255) & ~(size_t)255;
    for (int pass = 0; pass < 2; ++pass) {
        size_t held = 0;
        for (auto& c : d->chunks) {
            if (c.cap - c.used >= bytes) {
                *out = c.base + c.used;
                c.used += bytes;
                return ssdseg_poison_region(ctx, *out, bytes);
            }
            held += c.cap;
        }
        // every slab handed out so far has its column sum recorded (each entry point records it before it asks again), so a join
        // frees the whole arena.  Only from the main stream: the join there first waits for the side stream's slabs and readers.
        if (pass > 0 || held < arena_cap() || d->pending.empty() || ctx->side_on) break;
        int rc = ssdseg_join(ctx);
        if (rc) return rc;
    }
    ssdseg_defer::Chunk c;
    c.cap = bytes > ((size_t)256 << 20) ? bytes : ((size_t)256 << 20);
    c.used = bytes;
    void* p = nullptr;
    SSDSEG_HIP(hipMalloc(&p, c.cap));
    c.base = (char*)p;
    d->chunks.push_back(c);
    *out = p;
    return ssdseg_poison_region(ctx, p, bytes);
}

static int colsum_rc(int nparts, long long len) {
    // wide tables (weight-gradient slabs: thousands of columns) fill the chip with 32-column blocks as well, and those read whole
    // 128-byte lines of every partial row instead of 32-byte pieces (SSDSEG_COLSUM_RC=8 restores the narrow blocks for A/B runs)
    return (len >= 4096 && !env_is("SSDSEG_COLSUM_RC", '8')) ? 32 : reduce_rc(nparts, len);
}

int ssdseg_colsum(ssdseg_ctx* ctx, const float* part, int nparts, long long len, float* out) {
    const int rc = colsum_rc(nparts, len);
    ssdseg_defer* d = ctx->defer;
    if (d != nullptr && d->on && d->hold == 0 && defer_owns(d, part)) {
        // a destination recorded twice before a flush (an op repeated by a profiling script): the column sum OVERWRITES its
        // destination, so the later table supersedes the earlier one -- drop the earlier entry
        for (size_t i = 0; i < d->pending.size(); ++i)
            if (d->pending[i].out == out) {
                d->pending_bytes -= 4.0 * d->pending[i].nparts * (double)d->pending[i].len;
                d->pending.erase(d->pending.begin() + i);
                break;
            }
        ColsumEntry e;
        e.part = part; e.out = out; e.nparts = nparts; e.len = (int)len; e.rc = rc; e.block_begin = 0;
        d->pending.push_back(e);
        d->pending_bytes += 4.0 * nparts * (double)len;
        return 0;
    }
    const dim3 grid(cdiv(len, rc)), block(rc, RTHREADS / rc);
    for_rc(rc, [&](auto shape) {
        SSDSEG_LAUNCH_NAMED(ctx, "colsum_kernel", 4.0 * nparts * len, 0.0, colsum_kernel<decltype(shape)::value>, grid, block, 0, part, nparts,
                            (int)len, out);
    });
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_colsum_flush(ssdseg_ctx* ctx) {
    ssdseg_defer* d = ctx->defer;
    if (d == nullptr) return 0;
    if (d->pending.empty()) {
        for (auto& c : d->chunks) c.used = 0;
        return 0;
    }
    // called with the side stream joined and launches going to the main stream: every slab is complete in stream order
    int blocks = 0;
    for (auto& e : d->pending) {
        e.block_begin = blocks;
        blocks += cdiv(e.len, e.rc);
    }
    const size_t n = d->pending.size();
    if (n > d->d_cap) {
        SSDSEG_HIP(hipStreamSynchronize(ctx->stream));
        if (d->d_table) SSDSEG_HIP(hipFree(d->d_table));
        d->d_table = nullptr;
        d->d_cap = 0;
        void* p = nullptr;
        SSDSEG_HIP(hipMalloc(&p, (n + 64) * sizeof(ColsumEntry)));
        d->d_table = (ColsumEntry*)p;
        d->d_cap = n + 64;
        d->uploaded.clear();
    }
    // a training loop repeats the same pass: same arena offsets, same table -> nothing to upload after the first step
    const bool same = d->uploaded.size() == n && memcmp(d->uploaded.data(), d->pending.data(), n * sizeof(ColsumEntry)) == 0;
    if (!same) {
        d->uploaded = d->pending;     // (pageable source: the runtime has staged it when the call returns)
        SSDSEG_HIP(hipMemcpyAsync(d->d_table, d->uploaded.data(), n * sizeof(ColsumEntry), hipMemcpyHostToDevice, ctx->stream));
    }
    SSDSEG_LAUNCH(ctx, d->pending_bytes, 0.0, colsum_batch_kernel, dim3((unsigned)blocks), dim3(RTHREADS), 0, d->d_table, (int)n);
    d->pending.clear();
    d->pending_bytes = 0.0;
    for (auto& c : d->chunks) c.used = 0;     // the next pass's slabs are written by kernels queued behind this launch
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

void ssdseg_defer_hold(ssdseg_ctx* ctx, int delta) {
    if (ctx->defer != nullptr) ctx->defer->hold += delta;
}

void ssdseg_defer_destroy(ssdseg_ctx* ctx) {
    ssdseg_defer* d = ctx->defer;
    if (d == nullptr) return;
    for (auto& c : d->chunks) (void)hipFree(c.base);
    if (d->d_table) (void)hipFree(d->d_table);
    delete d;
    ctx->defer = nullptr;
}

extern "C" {

int ssdseg_colsum_defer(ssdseg_ctx* ctx, int enabled) {
    SSDSEG_ARG(ctx != nullptr, 1);
    if (ctx->defer == nullptr) {
        if (!enabled) return 0;
        ctx->defer = new ssdseg_defer();
    }
    if (!enabled) {
        int rc = ssdseg_join(ctx);      // flushes what is pending
        if (rc) return rc;
    }
    ctx->defer->on = enabled != 0;
    return 0;
}

}  // extern "C"
