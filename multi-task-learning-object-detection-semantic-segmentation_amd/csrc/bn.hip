// BatchNormalization (training mode) pieces that are not fused into a conv kernel, plus small elementwise helpers.
// Keras BatchNormalization: axis -1, eps 1e-3, momentum 0.99 (reference models.py:66,89,111; blocks.py:29,...;
// semantics SURVEY.md App. B.3).  All reductions are two-level with a fixed summation order (deterministic).
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int MAX_PARTS = 1024;

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

template <int RC>
__global__ void __launch_bounds__(RTHREADS) bn_finalize_kernel(const float* __restrict__ stats, int nparts, int c, double count,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
                                   float* __restrict__ moving_mean, float* __restrict__ moving_var, float* __restrict__ mean_out,
                                   float* __restrict__ invstd_out, float* __restrict__ scale, float* __restrict__ shift, int training) {
    __shared__ double red[2 * (RTHREADS / RC) * (RC + 1)];
    const int ch = blockIdx.x * RC + threadIdx.x;
    double tot[2] = {0.0, 0.0};
    if (training) reduce_parts<2, RC>(stats, nparts, c, ch, tot, red);
    if (threadIdx.y != 0 || ch >= c) return;
    double mean, var;
    if (training) {
        mean = tot[0] / count;
        var = tot[1] / count - mean * mean;
        if (var < 0.0) var = 0.0;
        if (moving_mean != nullptr) {
            const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
            moving_mean[ch] = (float)((double)moving_mean[ch] * momentum + mean * (1.0 - (double)momentum));
            moving_var[ch] = (float)((double)moving_var[ch] * momentum + unbiased * (1.0 - (double)momentum));
        }
    } else {
        mean = (double)moving_mean[ch];
        var = (double)moving_var[ch];
    }
    const double invstd = 1.0 / sqrt(var + (double)eps);
    if (mean_out) mean_out[ch] = (float)mean;
    if (invstd_out) invstd_out[ch] = (float)invstd;
    scale[ch] = (float)((double)gamma[ch] * invstd);
    shift[ch] = (float)((double)beta[ch] - mean * (double)gamma[ch] * invstd);
}

struct RowGeom {
    long long m;
    int c, cv;
};


__device__ __forceinline__ float4 reduce_over_y(float4 v, float4* red) {
    __syncthreads();
    red[threadIdx.y * blockDim.x + threadIdx.x] = v;
    __syncthreads();
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.y == 0)
        for (int y = 0; y < (int)blockDim.y; ++y) add4(r, red[y * blockDim.x + threadIdx.x]);
    return r;
}

// per-channel (sum, sumsq) of x[m][c]
__global__ void __launch_bounds__(512) channel_stats_kernel(const float* __restrict__ x, int ld, RowGeom g, float* __restrict__ stats) {
    extern __shared__ float4 red[];
    const int cvi = blockIdx.y * blockDim.x + threadIdx.x;
    const bool active = cvi < g.cv;
    float4 s = f4(0.f), q = f4(0.f);
    if (active) {
        for (long long r = (long long)blockIdx.x * blockDim.y + threadIdx.y; r < g.m; r += (long long)gridDim.x * blockDim.y) {
            const float4 v = ld4(x + r * ld + cvi * 4);
            add4(s, v);
            q.x = fmaf(v.x, v.x, q.x); q.y = fmaf(v.y, v.y, q.y); q.z = fmaf(v.z, v.z, q.z); q.w = fmaf(v.w, v.w, q.w);
        }
    }
    float4 a = reduce_over_y(s, red);
    float4 b = reduce_over_y(q, red);
    if (threadIdx.y == 0 && active) {
        float* row = stats + (long long)blockIdx.x * 2 * g.c;
        st4(row + cvi * 4, a);
        st4(row + g.c + cvi * 4, b);
    }
}

// partial (sum mask*g, sum mask*g*xhat) per channel
__global__ void __launch_bounds__(512) bn_bwd_partial_kernel(const float* __restrict__ gg, int ldg, const float* __restrict__ y, int ldy,
                                                             RowGeom g, const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd, int act,
                                                             float* __restrict__ part) {
    extern __shared__ float4 red[];
    const int cvi = blockIdx.y * blockDim.x + threadIdx.x;
    const bool active = cvi < g.cv;
    float4 sb = f4(0.f), sg = f4(0.f);
    if (active) {
        const float4 sc = ld4(scale + cvi * 4), sh = ld4(shift + cvi * 4), mu = ld4(mean + cvi * 4), is = ld4(invstd + cvi * 4);
        for (long long r = (long long)blockIdx.x * blockDim.y + threadIdx.y; r < g.m; r += (long long)gridDim.x * blockDim.y) {
            const float4 gv = ld4(gg + r * ldg + cvi * 4);
            const float4 yv = ld4(y + r * ldy + cvi * 4);
            float4 mg;
            mg.x = gv.x * act_mask(fmaf(sc.x, yv.x, sh.x), act);
            mg.y = gv.y * act_mask(fmaf(sc.y, yv.y, sh.y), act);
            mg.z = gv.z * act_mask(fmaf(sc.z, yv.z, sh.z), act);
            mg.w = gv.w * act_mask(fmaf(sc.w, yv.w, sh.w), act);
            add4(sb, mg);
            sg.x = fmaf(mg.x, (yv.x - mu.x) * is.x, sg.x);
            sg.y = fmaf(mg.y, (yv.y - mu.y) * is.y, sg.y);
            sg.z = fmaf(mg.z, (yv.z - mu.z) * is.z, sg.z);
            sg.w = fmaf(mg.w, (yv.w - mu.w) * is.w, sg.w);
        }
    }
    float4 a = reduce_over_y(sb, red);
    float4 b = reduce_over_y(sg, red);
    if (threadIdx.y == 0 && active) {
        float* row = part + (long long)blockIdx.x * 2 * g.c;
        st4(row + cvi * 4, a);
        st4(row + g.c + cvi * 4, b);
    }
}

template <int RC>
__global__ void __launch_bounds__(RTHREADS) bn_bwd_finalize_kernel(const float* __restrict__ part, int nparts, int c, double count,
                                       const float* __restrict__ scale, const float* __restrict__ mean, const float* __restrict__ invstd,
                                       float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ k1, float* __restrict__ k0) {
    __shared__ double red[2 * (RTHREADS / RC) * (RC + 1)];
    const int ch = blockIdx.x * RC + threadIdx.x;
    double tot[2] = {0.0, 0.0};
    reduce_parts<2, RC>(part, nparts, c, ch, tot, red);
    if (threadIdx.y != 0 || ch >= c) return;
    const double db = tot[0], dg = tot[1];
    if (dgamma) dgamma[ch] = (float)dg;
    if (dbeta) dbeta[ch] = (float)db;
    const double s = scale[ch], is = invstd[ch], mu = mean[ch];
    k1[ch] = (float)(-s * dg * is / count);
    k0[ch] = (float)(s * (dg * is * mu - db) / count);
}

// out[l] = sum_p part[p][l]
template <int RC>
__global__ void __launch_bounds__(RTHREADS) colsum_kernel(const float* __restrict__ part, int nparts, int len, float* __restrict__ out) {
    __shared__ double red[(RTHREADS / RC) * (RC + 1)];
    const int l = blockIdx.x * RC + threadIdx.x;
    double tot[1] = {0.0};
    reduce_parts<1, RC, 8>(part, nparts, len, l, tot, red);
    if (threadIdx.y == 0 && l < len) out[l] = (float)tot[0];
}

// Deferred column sums: every weight-gradient slab table of a backward pass in ONE launch.  Block b belongs to the entry whose
// block range contains it and does there exactly what a colsum_kernel<rc> block does (same lanes per column, same chains, same
// fold), so a gradient is the same bits whether its column sum was launched on its own or rides in the batch.
struct ColsumEntry {
    const float* part;
    float* out;
    int nparts, len, rc, block_begin;
};

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
    double tot[1] = {0.0};
    if (e.rc == 2) {
        const int tx = t & 1, ty = t >> 1, l = lb * 2 + tx;
        reduce_parts<1, 2, 8>(e.part, e.nparts, e.len, l, tot, red, tx, ty);
        if (ty == 0 && l < e.len) e.out[l] = (float)tot[0];
    } else if (e.rc == 8) {
        const int tx = t & 7, ty = t >> 3, l = lb * 8 + tx;
        reduce_parts<1, 8, 8>(e.part, e.nparts, e.len, l, tot, red, tx, ty);
        if (ty == 0 && l < e.len) e.out[l] = (float)tot[0];
    } else {
        const int tx = t & 31, ty = t >> 5, l = lb * 32 + tx;
        reduce_parts<1, 32, 8>(e.part, e.nparts, e.len, l, tot, red, tx, ty);
        if (ty == 0 && l < e.len) e.out[l] = (float)tot[0];
    }
}

__global__ void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                int ldx, const float* __restrict__ rx, const float* __restrict__ rscale, const float* __restrict__ rshift,
                                int ract, int ldr, float* __restrict__ out, int ldo, long long m, int cv) {
    const long long total = m * cv;
    const bool aff = scale != nullptr, raff = rscale != nullptr;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cv;
        const int c0 = (int)(i % cv) * 4;
        float4 s = f4(0.f), t = f4(0.f);
        if (aff) { s = ld4(scale + c0); t = ld4(shift + c0); }
        float4 v = view_apply4(ld4(x + r * ldx + c0), s, t, aff, act);
        if (rx) {
            float4 rs = f4(0.f), rt = f4(0.f);
            if (raff) { rs = ld4(rscale + c0); rt = ld4(rshift + c0); }
            add4(v, view_apply4(ld4(rx + r * ldr + c0), rs, rt, raff, ract));
        }
        st4(out + r * ldo + c0, v);
    }
}

__global__ void axpby_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd, long long m, int cv, float a, float b) {
    const long long total = m * cv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cv;
        const int c0 = (int)(i % cv) * 4;
        float4 s = ld4(src + r * lds + c0);
        float4 v;
        if (b != 0.f) {
            const float4 d = ld4(dst + r * ldd + c0);
            v = make_float4(fmaf(a, s.x, b * d.x), fmaf(a, s.y, b * d.y), fmaf(a, s.z, b * d.z), fmaf(a, s.w, b * d.w));
        } else {
            v = make_float4(a * s.x, a * s.y, a * s.z, a * s.w);
        }
        st4(dst + r * ldd + c0, v);
    }
}

// g <- dy = scale*mask(scale*y+shift)*g + k1*y + k0 in place (float4 per thread): materialises a BatchNorm-backward gradient view
__global__ void gview_materialize_kernel(float* __restrict__ g, int ldg, const float* __restrict__ y, int ldy, const float* __restrict__ scale,
                                         const float* __restrict__ shift, const float* __restrict__ k1, const float* __restrict__ k0, int act,
                                         long long m, int cv) {
    const long long total = m * cv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cv;
        const int c0 = (int)(i % cv) * 4;
        const float4 v = gview_apply4(ld4(g + r * ldg + c0), ld4(y + r * ldy + c0), ld4(scale + c0), ld4(shift + c0), ld4(k1 + c0), ld4(k0 + c0), act);
        st4(g + r * ldg + c0, v);
    }
}

struct RowLaunch {
    dim3 grid, block;
    size_t lds;
};

void row_launch(long long m, int c, RowGeom* g, RowLaunch* l) {
    g->m = m; g->c = c; g->cv = c / 4;
    int bx = g->cv < 256 ? g->cv : 256;
    int by = 512 / bx;
    if (by > 64) by = 64;
    long long want = (m + (long long)by * 8 - 1) / ((long long)by * 8);  // >= 8 rows per thread
    const char* pe = getenv("SSDSEG_BN_PARTS");       // (A/B runs) cap of partial rows of the streaming reductions
    const int maxp = pe != nullptr && atoi(pe) >= 64 && atoi(pe) <= MAX_PARTS ? atoi(pe) : MAX_PARTS;
    int gx = (int)(want < maxp ? want : maxp);
    if (gx < 1) gx = 1;
    l->block = dim3(bx, by, 1);
    l->grid = dim3(gx, cdiv(g->cv, bx), 1);
    l->lds = (size_t)bx * by * sizeof(float4);
}

int ew_blocks(long long total) {
    long long b = (total + 255) / 256;
    return (int)(b < 4096 ? (b < 1 ? 1 : b) : 4096);
}

}  // namespace

// shared with other translation units: out[l] = sum over nparts rows of part[p][l]
int ssdseg_bn_bwd_finalize_launch(ssdseg_ctx* ctx, const float* part, int nparts, int c, double count, const float* scale,
                                  const float* mean, const float* invstd, float* dgamma, float* dbeta, float* k1, float* k0) {
    const int rcw = reduce_rc(nparts, c);
    const dim3 fgrid(cdiv(c, rcw)), fblock(rcw, RTHREADS / rcw);
#define SSDSEG_BNBF(RCV)                                                                                                              \
    SSDSEG_LAUNCH_NAMED(ctx, "bn_bwd_finalize_kernel", 8.0 * nparts * c, 0.0, bn_bwd_finalize_kernel<RCV>, fgrid, fblock, 0, part, nparts, c, \
                        count, scale, mean, invstd, dgamma, dbeta, k1, k0)
    if (rcw == 2) SSDSEG_BNBF(2);
    else if (rcw == 8) SSDSEG_BNBF(8);
    else SSDSEG_BNBF(32);
#undef SSDSEG_BNBF
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------- deferred column sums
// Nothing reads a weight gradient before the optimizer (or the all-reduce in front of it), so the ~80 column sums that fold the
// partial slabs of the weight-gradient kernels need not be ~80 launches scattered over the backward pass: while deferral is on,
// the slabs live in a persistent arena (ssdseg_partials), ssdseg_colsum only records (slab table, destination), and the first
// ssdseg_join afterwards -- the engine joins the side stream at the end of backward() -- folds them all with one launch.
#include <vector>

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
    const char* e = getenv("SSDSEG_COLSUM_ARENA_MB");
    return (e != nullptr && atoll(e) > 0 ? (size_t)atoll(e) : (size_t)4096) << 20;
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
    const char* e = getenv("SSDSEG_COLSUM_RC");
    return (len >= 4096 && !(e != nullptr && e[0] == '8')) ? 32 : reduce_rc(nparts, len);
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
    if (rc == 2) SSDSEG_LAUNCH_NAMED(ctx, "colsum_kernel", 4.0 * nparts * len, 0.0, colsum_kernel<2>, grid, block, 0, part, nparts, (int)len, out);
    else if (rc == 8) SSDSEG_LAUNCH_NAMED(ctx, "colsum_kernel", 4.0 * nparts * len, 0.0, colsum_kernel<8>, grid, block, 0, part, nparts, (int)len, out);
    else SSDSEG_LAUNCH_NAMED(ctx, "colsum_kernel", 4.0 * nparts * len, 0.0, colsum_kernel<32>, grid, block, 0, part, nparts, (int)len, out);
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

int ssdseg_bn_finalize(ssdseg_ctx* ctx, const float* stats, int nparts, int c, double count, const float* gamma,
                       const float* beta, float eps, float momentum, float* moving_mean, float* moving_var, float* mean,
                       float* invstd, float* scale, float* shift, int training) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(!training || (stats != nullptr && nparts > 0), 2);
    SSDSEG_ARG(c > 0, 4);
    SSDSEG_ARG(!training || count >= 1.0, 5);
    SSDSEG_ARG(gamma != nullptr, 6);
    SSDSEG_ARG(beta != nullptr, 7);
    SSDSEG_ARG(training || (moving_mean != nullptr && moving_var != nullptr), 10);
    SSDSEG_ARG((moving_mean == nullptr) == (moving_var == nullptr), 11);
    SSDSEG_ARG(scale != nullptr, 14);
    SSDSEG_ARG(shift != nullptr, 15);
    const int rc = training ? reduce_rc(nparts, c) : 32;
    const dim3 grid(cdiv(c, rc)), block(rc, RTHREADS / rc);
#define SSDSEG_BNF(RCV)                                                                                                                     \
    SSDSEG_LAUNCH_NAMED(ctx, "bn_finalize_kernel", 8.0 * nparts * c, 0.0, bn_finalize_kernel<RCV>, grid, block, 0, stats, nparts, c, count, gamma, \
                        beta, eps, momentum, moving_mean, moving_var, mean, invstd, scale, shift, training)
    if (rc == 2) SSDSEG_BNF(2);
    else if (rc == 8) SSDSEG_BNF(8);
    else SSDSEG_BNF(32);
#undef SSDSEG_BNF
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_channel_stats_parts(int m, int c, int* nparts_host) {
    SSDSEG_ARG(m > 0, 1);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 2);
    SSDSEG_ARG(nparts_host != nullptr, 3);
    RowGeom g;
    RowLaunch l;
    row_launch(m, c, &g, &l);
    *nparts_host = (int)l.grid.x;
    return 0;
}

int ssdseg_channel_stats(ssdseg_ctx* ctx, const float* x, int ld, int m, int c, float* stats) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(x != nullptr, 2);
    SSDSEG_ARG(ld >= c && ld % 4 == 0, 3);
    SSDSEG_ARG(m > 0, 4);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 5);
    SSDSEG_ARG(stats != nullptr, 6);
    RowGeom g;
    RowLaunch l;
    row_launch(m, c, &g, &l);
    SSDSEG_LAUNCH(ctx, 4.0 * m * c, 0.0, channel_stats_kernel, l.grid, l.block, l.lds, x, ld, g, stats);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_bn_apply(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_view* residual, int ldr, float* out, int ldo,
                    int m, int c) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= c && ldx % 4 == 0, 3);
    SSDSEG_ARG(residual == nullptr || (residual->x != nullptr && ((residual->scale == nullptr) == (residual->shift == nullptr))), 4);
    SSDSEG_ARG(residual == nullptr || (ldr >= c && ldr % 4 == 0), 5);
    SSDSEG_ARG(out != nullptr, 6);
    SSDSEG_ARG(ldo >= c && ldo % 4 == 0, 7);
    SSDSEG_ARG(m > 0, 8);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 9);
    const long long total = (long long)m * (c / 4);
    SSDSEG_LAUNCH(ctx, 4.0 * m * c * (residual ? 3 : 2), 0.0, bn_apply_kernel, dim3(ew_blocks(total)), dim3(256), 0, in->x, in->scale, in->shift, in->act, ldx,
                       residual ? residual->x : nullptr, residual ? residual->scale : nullptr, residual ? residual->shift : nullptr,
                       residual ? residual->act : 0, ldr, out, ldo, (long long)m, c / 4);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_bn_bwd_reduce(ssdseg_ctx* ctx, const float* g, int ldg, const float* y, int ldy, int m, int c, const float* scale,
                         const float* shift, const float* mean, const float* invstd, int act, float* dgamma, float* dbeta,
                         float* k1, float* k0) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(g != nullptr, 2);
    SSDSEG_ARG(ldg >= c && ldg % 4 == 0, 3);
    SSDSEG_ARG(y != nullptr, 4);
    SSDSEG_ARG(ldy >= c && ldy % 4 == 0, 5);
    SSDSEG_ARG(m > 0, 6);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 7);
    SSDSEG_ARG(scale && shift && mean && invstd, 8);
    SSDSEG_ARG(k1 != nullptr && k0 != nullptr, 15);
    RowGeom rg;
    RowLaunch l;
    row_launch(m, c, &rg, &l);
    void* ws;
    int rc = ssdseg_workspace(ctx, (size_t)l.grid.x * 2 * c * sizeof(float), &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, 8.0 * m * c, 0.0, bn_bwd_partial_kernel, l.grid, l.block, l.lds, g, ldg, y, ldy, rg, scale, shift, mean, invstd, act,
                       (float*)ws);
    SSDSEG_LAUNCH_CHECK();
    return ssdseg_bn_bwd_finalize_launch(ctx, (const float*)ws, (int)l.grid.x, c, (double)m, scale, mean, invstd, dgamma, dbeta, k1, k0);
}

int ssdseg_gview_materialize(ssdseg_ctx* ctx, const ssdseg_gview* dy, int ld, int m, int c) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr && dy->y != nullptr && dy->scale && dy->shift && dy->k1 && dy->k0, 2);
    SSDSEG_ARG(ld >= c && ld % 4 == 0, 3);
    SSDSEG_ARG(m > 0, 4);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 5);
    const long long total = (long long)m * (c / 4);
    SSDSEG_LAUNCH(ctx, 12.0 * m * c, 0.0, gview_materialize_kernel, dim3(ew_blocks(total)), dim3(256), 0, (float*)dy->g, ld, dy->y, ld, dy->scale,
                  dy->shift, dy->k1, dy->k0, dy->act, (long long)m, c / 4);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_axpby(ssdseg_ctx* ctx, const float* src, int lds, float* dst, int ldd, int m, int c, float a, float b) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(src != nullptr, 2);
    SSDSEG_ARG(lds >= c && lds % 4 == 0, 3);
    SSDSEG_ARG(dst != nullptr, 4);
    SSDSEG_ARG(ldd >= c && ldd % 4 == 0, 5);
    SSDSEG_ARG(m > 0, 6);
    SSDSEG_ARG(c > 0 && c % 4 == 0, 7);
    const long long total = (long long)m * (c / 4);
    SSDSEG_LAUNCH(ctx, 4.0 * m * c * (b != 0.f ? 3 : 2), 0.0, axpby_kernel, dim3(ew_blocks(total)), dim3(256), 0, src, lds, dst, ldd, (long long)m, c / 4, a, b);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
