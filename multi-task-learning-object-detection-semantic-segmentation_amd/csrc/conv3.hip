// Dense 3x3 stride-1 SAME convolution (DeepLabV3+ decoder, reference blocks.py:117-127): every form of it and the ssdseg_conv3x3_*
// entry points that choose between them.
//   narrow (cout <= 8)      tap-expanded columns around the pointwise GEMMs of gemm.hip        (this file)
//   halo tile               conv3_tile.h (forward, input gradient), conv3_wgrad_tile.h (weight gradient)
//   Winograd F(2x2, 3x3)    conv3_wino.h, conv3_wino_wgrad.h          F(4x4, 3x3)   conv3_wino4.h
//   nine taps in one pass   conv3_wgrad.h (weight gradient with a BatchNorm gradient view)
//   implicit GEMM           gemm_rowA_kernel<.., LD = 1> / gemm_wgrad_kernel per tap in gemm.hip, reached through gemm_internal.h
#include "gemm_internal.h"
#include <stdlib.h>
#include <vector>

namespace {

#include "conv3_wgrad.h"
#include "conv3_tile.h"
#include "conv3_wgrad_tile.h"
#include "conv3_wino.h"
#include "conv3_wino4.h"
#include "conv3_wino_wgrad.h"

// ------------------------------------------------------------------------------------------------ narrow 3x3 conv
// Dense 3x3 conv with very few output channels (the 256 -> 4 mask-logits conv at 120x160: 75 % of the implicit-GEMM tile
// is padding and every input pixel is gathered nine times: 1.2 / 1.4 / 0.35 ms for fwd / dW / dx).  Rewritten over
// TAP-EXPANDED columns, everything heavy becomes a pointwise GEMM that reads the wide tensor exactly once:
//   fwd : z[m][tap*co + o] = sum_c a[m][c] W[tap][c][o]   (GEMM, N = 9*co)     y[m][o] = sum_tap z[m + d(tap)][tap*co + o]
//   bwd : dz[m][tap*co + o] = dy[m - d(tap)][o]            (shifted copy)       dx = dz * W2^T,  dW2 = a^T * dz  (GEMMs)
// with d(tap) = (kh - 1, kw - 1) and W2[c][tap*co + o] = W[tap][c][o].
constexpr int C3N_MAX_COUT = 8;

bool conv3_narrow(int cin, int cout) {
    const char* e = getenv("SSDSEG_CONV3_NARROW");   // "0": the implicit-GEMM kernels (A/B measurements, parity tests)
    return !(e != nullptr && e[0] == '0') && cout <= C3N_MAX_COUT && cin >= 4 * cout;
}

__global__ void conv3n_pack_w_kernel(const float* __restrict__ w, float* __restrict__ w2, int cin, int cout, int reverse) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over [9][cin][cout]
    if (i >= 9 * cin * cout) return;
    const int o = i % cout, c = (i / cout) % cin, tap = i / (cout * cin);
    const int j = c * 9 * cout + tap * cout + o;
    if (reverse) const_cast<float*>(w)[i] = w2[j];   // dW2 -> dW
    else w2[j] = w[i];
}

// y[m][o] = sum_tap z[m + d(tap)][tap*co + o]; optional BN statistics: one partial row (sum, sumsq per channel) per block
__global__ void __launch_bounds__(256) conv3n_tapsum_kernel(const float* __restrict__ z, float* __restrict__ y, int n, int h, int w, int cv,
                                                            float* __restrict__ stats) {
    __shared__ float4 red[2][256];
    // (32-bit index arithmetic: the launcher guarantees n*h*w*9*cv < 2^31 -- 64-bit divisions cost more than the kernel's traffic)
    const int total = n * h * w * cv;
    const int ldz = 9 * cv * 4;
    float4 ssum = f4(0.f), ssq = f4(0.f);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int c4 = i % cv;
        int r = i / cv;
        const int x = r % w; r /= w;
        const int yy = r % h;
        const long long img = r / h;
        float4 acc = f4(0.f);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int sy = yy + tap / 3 - 1, sx = x + tap % 3 - 1;
            if (sy >= 0 && sy < h && sx >= 0 && sx < w) add4(acc, ld4(z + ((img * h + sy) * w + sx) * ldz + (tap * cv + c4) * 4));
        }
        st4(y + (long long)i * 4, acc);
        add4(ssum, acc);
        ssq.x = fmaf(acc.x, acc.x, ssq.x); ssq.y = fmaf(acc.y, acc.y, ssq.y); ssq.z = fmaf(acc.z, acc.z, ssq.z); ssq.w = fmaf(acc.w, acc.w, ssq.w);
    }
    if (stats == nullptr) return;
    red[0][threadIdx.x] = ssum; red[1][threadIdx.x] = ssq;   // thread t always has channel vector t % cv (256 % cv == 0)
    __syncthreads();
    for (int off = 128; off >= cv; off >>= 1) {
        if ((int)threadIdx.x < off) { add4(red[0][threadIdx.x], red[0][threadIdx.x + off]); add4(red[1][threadIdx.x], red[1][threadIdx.x + off]); }
        __syncthreads();
    }
    if ((int)threadIdx.x < cv) {
        st4(stats + ((long long)blockIdx.x * 2 + 0) * cv * 4 + threadIdx.x * 4, red[0][threadIdx.x]);
        st4(stats + ((long long)blockIdx.x * 2 + 1) * cv * 4 + threadIdx.x * 4, red[1][threadIdx.x]);
    }
}

// dz[m][tap*co + o] = dy[m - d(tap)][o] (0 outside the image), dy formed from the gradient view on the way
__global__ void __launch_bounds__(256) conv3n_shift_kernel(const float* __restrict__ g, const float* __restrict__ yv, const float* __restrict__ gs,
                                                           const float* __restrict__ gt, const float* __restrict__ gk1,
                                                           const float* __restrict__ gk0, int gact, float* __restrict__ dz, int n, int h, int w,
                                                           int cv) {
    const int total = n * h * w * 9 * cv;      // < 2^31 (launcher)
    const bool aff = gs != nullptr;
    const float* yp = aff ? yv : g;
    const int act = aff ? gact : SSDSEG_ACT_NONE;
    float4 s = f4(1.f), t = f4(0.f), k1 = f4(0.f), k0 = f4(0.f);
    const int cfix = threadIdx.x % cv;           // 256 % cv == 0 and the grid stride is a multiple of 256: a thread keeps its channel vector
    if (aff) { s = ld4(gs + cfix * 4); t = ld4(gt + cfix * 4); k1 = ld4(gk1 + cfix * 4); k0 = ld4(gk0 + cfix * 4); }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int c4 = cfix;
        int r = i / cv;
        const int tap = r % 9; r /= 9;
        const int x = r % w; r /= w;
        const int yy = r % h;
        const long long img = r / h;
        const int sy = yy - (tap / 3 - 1), sx = x - (tap % 3 - 1);
        float4 v = f4(0.f);
        if (sy >= 0 && sy < h && sx >= 0 && sx < w) {
            const long long o = (((img * h + sy) * w + sx) * cv + c4) * 4;
            v = gview_apply4(ld4(g + o), ld4(yp + o), s, t, k1, k0, act);
        }
        st4(dz + (long long)i * 4, v);
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Scratch of a narrow-form entry point, at the front of the workspace: W2 (or dW2) [cin][9*cout], then z (or dz) [m][9*cout].  While the
// nested pointwise GEMM runs, the entry point holds `bytes` through ctx->ws_reserved and the GEMM allocates BEHIND them (ssdseg_workspace
// honours ws_reserved: hence the head-room in the request).
struct Conv3nScratch {
    long long m;
    int nc, cv;
    size_t bytes;
    float *w2, *z;
};
// w != nullptr: also packs the weights into W2
int conv3n_reserve(ssdseg_ctx* ctx, const float* w, int n, int h, int wdt, int cin, int cout, Conv3nScratch* s) {
    s->m = (long long)n * h * wdt;
    s->nc = 9 * cout; s->cv = cout / 4;
    const size_t wb = align256((size_t)cin * s->nc * sizeof(float)), zb = align256((size_t)s->m * s->nc * sizeof(float));
    s->bytes = wb + zb;
    void* ws;
    int rc = ssdseg_workspace(ctx, s->bytes + s->bytes / 2 + ((size_t)64 << 20), &ws);
    if (rc) return rc;
    s->w2 = (float*)ws;
    s->z = (float*)((char*)ws + wb);
    if (w == nullptr) return 0;
    SSDSEG_LAUNCH(ctx, 8.0 * 9 * cin * cout, 0.0, conv3n_pack_w_kernel, dim3(cdiv(9 * cin * cout, 256)), dim3(256), 0, w, s->w2, cin, cout, 0);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
// s.z = dz[m][tap][o] = dy[m - d(tap)][o], dy formed from the gradient view on the way
int conv3n_shift(ssdseg_ctx* ctx, const ssdseg_gview* dy, const Conv3nScratch& s, int n, int h, int wdt, int cout) {
    const long long tot = s.m * 9 * s.cv;
    SSDSEG_ARG(tot < (1LL << 31), 6);       // 32-bit element indices in conv3n_shift_kernel
    SSDSEG_LAUNCH(ctx, 4.0 * s.m * (s.nc + (dy->scale ? 2.0 : 1.0) * cout), 0.0, conv3n_shift_kernel, dim3((unsigned)((tot + 255) / 256 < 8192 ? (tot + 255) / 256 : 8192)),
                  dim3(256), 0, dy->g, dy->y, dy->scale, dy->shift, dy->k1, dy->k0, dy->act, s.z, n, h, wdt, s.cv);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// dynamic LDS beyond 64 KiB has to be announced once per kernel (again when a call needs more than any before it)
template <auto KERNEL>
int conv3_announce_lds(size_t lds) {
    static size_t configured = 0;
    if (lds > configured) {
        SSDSEG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        configured = lds;
    }
    return 0;
}

// ---- halo-tile 3x3 conv (conv3_tile.h): geometry and launch
bool conv3_tile_enabled() {
    const char* e = getenv("SSDSEG_CONV3_TILE");   // "0": the implicit-GEMM kernels (A/B measurements, parity tests)
    return !(e != nullptr && e[0] == '0');
}
bool conv3_tile_fwd_ok(int cin, int cout) { return conv3_tile_enabled() && !conv3_narrow(cin, cout) && cin % C3T_KC == 0; }
// 32-bit buffer offsets: the streamed tensor (row stride ld) has to stay below 2^31 bytes
bool conv3_tile_fits(int n, int h, int w, int ld) { return (long long)n * h * w * ld * 4 < (1LL << 31); }

struct Conv3TGeom {
    int tiles_h, tiles_w, mtiles, ntiles_n, ncols, wn;
};
Conv3TGeom conv3t_geometry(int n, int h, int w, int nout) {
    Conv3TGeom g;
    g.tiles_h = cdiv(h, C3T_ROWS);
    g.tiles_w = cdiv(w, C3T_COLS);
    g.mtiles = n * g.tiles_h * g.tiles_w;
    g.ntiles_n = cdiv(nout, 160);
    g.ncols = (cdiv(nout, g.ntiles_n) + 3) / 4 * 4;
    g.wn = cdiv(g.ncols, 32);
    return g;
}

// what the halo-tile and the Winograd launchers take from an entry point; they fill in the weights, the tiling and the buffer extents
Conv3TArgs conv3t_args(const float* x, const float* cs, const float* ct, int act, int ldi, float* out, int ldo, int accumulate, float* stats, int n,
                       int h, int w, int cred, int nout) {
    Conv3TArgs t{};
    t.in = x; t.cs = cs; t.ct = ct; t.act = act; t.ldi = ldi;
    t.out = out; t.ldo = ldo; t.accumulate = accumulate;
    t.stats = stats;
    t.n = n; t.h = h; t.w = w; t.cred = cred; t.nout = nout;
    return t;
}

template <int WN>
int conv3t_launch_wn(ssdseg_ctx* ctx, const Conv3TArgs& a, const Conv3TGeom& g, double cost_bytes, double cost_flops) {
    const size_t lds = conv3t_lds_floats(WN, a.cred) * sizeof(float);
    if (int rc = conv3_announce_lds<&conv3_tile_kernel<WN>>(lds)) return rc;
    char kbuf[64];
    snprintf(kbuf, sizeof(kbuf), "conv3_tile_kernel<%d>%s", WN, a.flip ? " [bwd_data]" : " [fwd]");
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, (conv3_tile_kernel<WN>), dim3((unsigned)(g.mtiles * g.ntiles_n)), dim3(C3T_THREADS), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int conv3t_launch(ssdseg_ctx* ctx, Conv3TArgs a) {
    const Conv3TGeom g = conv3t_geometry(a.n, a.h, a.w, a.nout);
    a.tiles_h = g.tiles_h; a.tiles_w = g.tiles_w; a.ntiles_n = g.ntiles_n; a.ncols = g.ncols;
    a.in_bytes = (unsigned)((((long long)a.n * a.h * a.w - 1) * a.ldi + a.cred) * 4);
    a.wt_bytes = (unsigned)((long long)9 * a.nout * a.cred * 4);
    const double m = (double)a.n * a.h * a.w;
    const double cost_bytes = 4.0 * (m * a.cred + m * a.nout + 9.0 * a.cred * a.nout);   // X + Y + W
    const double cost_flops = 18.0 * m * a.cred * a.nout;
    switch (g.wn) {
        case 1: return conv3t_launch_wn<1>(ctx, a, g, cost_bytes, cost_flops);
        case 2: return conv3t_launch_wn<2>(ctx, a, g, cost_bytes, cost_flops);
        case 3: return conv3t_launch_wn<3>(ctx, a, g, cost_bytes, cost_flops);
        case 4: return conv3t_launch_wn<4>(ctx, a, g, cost_bytes, cost_flops);
        default: return conv3t_launch_wn<5>(ctx, a, g, cost_bytes, cost_flops);
    }
}

// ---- Winograd F(2x2, 3x3) form (conv3_wino.h).  SSDSEG_CONV3_WINOGRAD=0: the direct halo-tile kernels.
int conv3_wino_mode() {      // 0 off, 1 forced (any size; parity tests), 2 automatic
    const char* e = getenv("SSDSEG_CONV3_WINOGRAD");
    if (!conv3_tile_enabled()) return 0;
    return e == nullptr || e[0] == '\0' ? 2 : (e[0] == '0' ? 0 : 1);
}
// automatic: where the 16 transformed GEMMs fill the chip -- >= 64 output channels, a few hundred pixel tiles
bool conv3_wino_takes(int n, int h, int w, int cred, int nout) {
    const int mode = conv3_wino_mode();
    if (mode == 0 || cred % C3T_KC != 0 || wino_lds_floats(cred) * sizeof(float) > (size_t)160 * 1024) return false;
    return mode == 1 || (nout >= 64 && (long long)n * cdiv(h, C3T_ROWS) * cdiv(w, C3T_COLS) >= 256);
}

// ---- Winograd F(4x4, 3x3) form (conv3_wino4.h): forward / input gradient of the layers the F(2x2) form takes, where a tile
// geometry exists.  SSDSEG_CONV3_F4=0: never, =1: wherever it fits (parity tests); unset: the large layers.
struct Wino4Geom { int tr, tc, trs, tiles_h, tiles_w; };
bool wino4_geometry(int h, int w, Wino4Geom* g) {
    long long best = -1;
    for (int tc = 1; tc <= 11; ++tc)
        for (int tr = 1; tr * tc <= 32; ++tr) {
            if (4 * tr * (4 * tc + 2) > 2 * W4_THREADS) continue;      // strips x four 16-byte chunks: two tasks per thread
            int trs = 24 * W4_RL;
            while ((trs & 15) != (tc & 15)) ++trs;
            if (tr * trs + 15 > W4_QP_MAX) continue;            // (+ the round-up of the plane stride to 1 mod 16)
            const long long blocks = (long long)cdiv(h, 4 * tr) * cdiv(w, 4 * tc);
            // fewest blocks (every block costs a full 32-row MFMA pass); then the squarer patch (less halo)
            const long long key = blocks * 1024 + (tr > tc ? tr - tc : tc - tr);
            if (best < 0 || key < best) { best = key; *g = Wino4Geom{tr, tc, trs, cdiv(h, 4 * tr), cdiv(w, 4 * tc)}; }
        }
    return best >= 0;
}
// what the F(4x4) kernel can take, whatever the switches say: 16-channel steps, its LDS (and that of the F(2x2) form it stands in for)
// within 160 KiB, a tile geometry, U[cred / 8][36][npad][8] below 2^31 bytes
bool wino4_fits(int h, int w, int cred, int nout, Wino4Geom* g) {
    if (cred % 16 != 0 || wino_lds_floats(cred) * sizeof(float) > (size_t)160 * 1024 || wino4_lds_floats(cred) * sizeof(float) > (size_t)160 * 1024) return false;
    return wino4_geometry(h, w, g) && (long long)36 * cred * cdiv(nout, W4_NT) * W4_NT * 4 < (1LL << 31);
}
bool conv3_wino4_takes(int n, int h, int w, int cred, int nout) {
    const char* e = getenv("SSDSEG_CONV3_F4");
    if (e != nullptr && e[0] == '0') return false;
    Wino4Geom g;
    if (!conv3_wino_takes(n, h, w, cred, nout) || !wino4_fits(h, w, cred, nout, &g)) return false;
    if (e != nullptr && e[0] == '1') return true;
    // automatic: where every CU gets a few work items (pixel tile x 32-channel tile) -- the decoder conv of the full-size models
    return (long long)n * g.tiles_h * g.tiles_w * cdiv(nout, W4_NT) >= 2048;
}

int conv3_wino4_launch(ssdseg_ctx* ctx, const Conv3TArgs& a, const float* w, int cin, int cout, int mode) {
    Wino4Geom g;
    if (!wino4_geometry(a.h, a.w, &g)) return SSDSEG_EINVAL(6);
    void* ws;
    const int npad = cdiv(a.nout, W4_NT) * W4_NT;
    const size_t ubytes = (size_t)36 * a.cred * npad * sizeof(float);      // U[cred / 8][36][npad][8]
    int rc = ssdseg_workspace(ctx, ubytes, &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, 4.0 * (9 + 36) * cin * cout, 0.0, conv3_wino4_weights_kernel, dim3(cdiv(cout, 32), cdiv(cin, 32)), dim3(256), 0, w, (float*)ws, cin, cout, mode);
    SSDSEG_LAUNCH_CHECK();
    Wino4Args p{};
    p.in = a.in; p.cs = a.cs; p.ct = a.ct; p.act = a.act; p.ldi = a.ldi;
    p.u = (const float*)ws;
    p.out = a.out; p.ldo = a.ldo; p.accumulate = a.accumulate; p.stats = a.stats;
    p.n = a.n; p.h = a.h; p.w = a.w; p.cred = a.cred; p.nout = a.nout; p.npad = npad;
    p.tr = g.tr; p.tc = g.tc; p.trs = g.trs;
    p.qps = g.tr * g.trs;
    while ((p.qps & 15) != 1) ++p.qps; p.tiles_h = g.tiles_h; p.tiles_w = g.tiles_w; p.ntiles_n = npad / W4_NT;
    {
        const char* ge = getenv("SSDSEG_W4_GROUP");      // (A/B runs) channel tiles per group of the work order
        p.group = ge != nullptr ? atoi(ge) : 2;
        if (p.group < 1 || p.ntiles_n % p.group != 0) p.group = 1;
    }
    p.in_hp = a.in_hp ? a.in_hp : a.h; p.in_wp = a.in_hp ? a.in_wp : a.w;
    p.in_bytes = (unsigned)(((((long long)(a.n - 1) * p.in_hp + a.h - 1) * p.in_wp + a.w - 1) * a.ldi + a.cred) * 4);
    p.u_bytes = (unsigned)ubytes;
    {
        const long long ob = (((long long)a.n * a.h * a.w - 1) * a.ldo + a.nout) * 4;
        p.out_bytes = ob < (1LL << 31) ? (unsigned)ob : 0u;
        if (ob >= (1LL << 31) && !p.accumulate) p.accumulate = 2;      // 32-bit buffer offsets do not reach: plain stores
        const char* fe = getenv("SSDSEG_W4_PLAIN_STORES");              // (parity tests) that path at any size
        if (fe != nullptr && fe[0] == '1' && !p.accumulate) p.accumulate = 2;
    }
    p.trace = nullptr;
    const size_t lds = wino4_lds_floats(a.cred) * sizeof(float);
    if ((rc = conv3_announce_lds<&conv3_wino4_kernel<false>>(lds)) || (rc = conv3_announce_lds<&conv3_wino4_kernel<true>>(lds))) return rc;
    const double m = (double)a.n * a.h * a.w;
    const double cost_bytes = 4.0 * (m * a.cred + m * a.nout + 9.0 * a.cred * a.nout);   // X + Y + W
    // flops EXECUTED on the MFMA pipe: 36 positions x (m / 16) tiles x 2 cred nout = 4.5 m cred nout -- a quarter of the direct sum's 18
    const double cost_flops = 4.5 * m * a.cred * a.nout;
    const int mtiles = a.n * g.tiles_h * g.tiles_w;
    // persistent blocks: one per CU (154 KB of LDS each), a multiple of 8 so that every XCD walks one contiguous run of the items
    const long long items = (long long)mtiles * p.ntiles_n;
    int nblocks = ctx->num_cus;
    if (const char* e = getenv("SSDSEG_W4_BLOCKS")) nblocks = atoi(e) > 0 ? atoi(e) : nblocks;
    if (nblocks > items) nblocks = (int)items;
    if (nblocks >= 8 && items % 8 == 0) nblocks -= nblocks % 8;
    if (getenv("SSDSEG_W4_TRACE") != nullptr) { SSDSEG_HIP(hipMalloc((void**)&p.trace, (size_t)nblocks * 64 * 4 * 8)); SSDSEG_HIP(hipMemset(p.trace, 0, (size_t)nblocks * 64 * 4 * 8)); }
    const bool with_view = a.cs != nullptr || a.act != SSDSEG_ACT_NONE;
    char kbuf[64];
    snprintf(kbuf, sizeof(kbuf), "conv3_wino4_kernel<%s> [%s]", with_view ? "true" : "false", mode ? "bwd_data" : "fwd");
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    if (with_view)
        SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, conv3_wino4_kernel<true>, dim3((unsigned)nblocks), dim3(W4_THREADS), lds, p);
    else
        SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, conv3_wino4_kernel<false>, dim3((unsigned)nblocks), dim3(W4_THREADS), lds, p);
    SSDSEG_LAUNCH_CHECK();
    if (p.trace != nullptr) {       // measurement only: synchronous, prints to stderr
        std::vector<unsigned long long> h((size_t)nblocks * 64 * 4);
        SSDSEG_HIP(hipStreamSynchronize(ctx->stream));
        SSDSEG_HIP(hipMemcpy(h.data(), p.trace, h.size() * 8, hipMemcpyDeviceToHost));
        SSDSEG_HIP(hipFree(p.trace));
        const int per = (int)((items + nblocks - 1) / nblocks) < 64 ? (int)((items + nblocks - 1) / nblocks) : 64;
        for (int b : {0, 1, nblocks / 2, nblocks - 1}) {
            double loop = 0, epi = 0;
            for (int k = 0; k < per; ++k) {
                loop += (double)(h[((size_t)b * 64 + k) * 4 + 1] - h[((size_t)b * 64 + k) * 4 + 0]);
                epi += (double)(h[((size_t)b * 64 + k) * 4 + 2] - h[((size_t)b * 64 + k) * 4 + 1]);
            }
            const double gap = per > 1 ? ((double)(h[((size_t)b * 64 + per - 1) * 4 + 0] - h[((size_t)b * 64) * 4 + 0]) - (loop - (double)(h[((size_t)b * 64 + per - 1) * 4 + 1] - h[((size_t)b * 64 + per - 1) * 4 + 0])) ) / (per - 1) : 0;
            fprintf(stderr, "w4 trace block %3d: %d items, loop %.0f clk/item (%.0f per 16-channel step), loop end -> item end %.0f, loop end -> next loop start %.0f\n", b, per,
                    loop / per, loop / per / (a.cred / 16), epi / per, gap);
        }
    }
    return 0;
}

// a: in / view / out / stats / shape as for conv3t_launch; w = the layer's [3][3][cin][cout] weights; mode 0 forward, 1 input gradient
int conv3_wino_launch(ssdseg_ctx* ctx, Conv3TArgs a, const float* w, int cin, int cout, int mode) {
    if (conv3_wino4_takes(a.n, a.h, a.w, a.cred, a.nout)) return conv3_wino4_launch(ctx, a, w, cin, cout, mode);
    void* ws;
    const int npad = cdiv(a.nout, WINO_NT) * WINO_NT;
    const size_t ubytes = (size_t)16 * a.cred * npad * sizeof(float);      // U[cred / 8][16][npad][8]
    int rc = ssdseg_workspace(ctx, ubytes, &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, 4.0 * (9 + 16) * cin * cout, 0.0, conv3_wino_weights_kernel, dim3(cdiv(cout, 32), cdiv(cin, 32)), dim3(256), 0, w, (float*)ws, cin, cout, mode);
    SSDSEG_LAUNCH_CHECK();
    a.wt = (const float*)ws;
    a.tiles_h = cdiv(a.h, C3T_ROWS); a.tiles_w = cdiv(a.w, C3T_COLS); a.ntiles_n = cdiv(a.nout, WINO_NT); a.ncols = WINO_NT;
    if (a.in_hp == 0) { a.in_hp = a.h; a.in_wp = a.w; }
    // (the zero-bordered copy is entered at its pixel (1, 1): the last byte the kernel may touch is that of image pixel (h-1, w-1))
    a.in_bytes = (unsigned)(((((long long)(a.n - 1) * a.in_hp + a.h - 1) * a.in_wp + a.w - 1) * a.ldi + a.cred) * 4);
    a.wt_bytes = (unsigned)ubytes;
    const size_t lds = wino_lds_floats(a.cred) * sizeof(float);
    if ((rc = conv3_announce_lds<&conv3_wino_kernel<false>>(lds)) || (rc = conv3_announce_lds<&conv3_wino_kernel<true>>(lds))) return rc;
    const double m = (double)a.n * a.h * a.w;
    const double cost_bytes = 4.0 * (m * a.cred + m * a.nout + 9.0 * a.cred * a.nout);   // X + Y + W
    // flops EXECUTED on the MFMA pipe: 16 positions x (m / 4) tiles x 2 cred nout = 8 m cred nout -- 16/36 of the direct convolution's
    // 18 m cred nout (bench.py reports that figure beside it as `direct_equivalent`; the roofline fraction uses the executed ones)
    const double cost_flops = 8.0 * m * a.cred * a.nout;
    const int mtiles = a.n * a.tiles_h * a.tiles_w;
    const bool with_view = a.cs != nullptr || a.act != SSDSEG_ACT_NONE;
    char kbuf[64];
    snprintf(kbuf, sizeof(kbuf), "conv3_wino_kernel<%s> [%s]", with_view ? "true" : "false", mode ? "bwd_data" : "fwd");   // symbol as rocprofv3 spells it + role
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    if (with_view)
        SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, conv3_wino_kernel<true>, dim3((unsigned)(mtiles * a.ntiles_n)), dim3(C3T_THREADS), lds, a);
    else
        SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, conv3_wino_kernel<false>, dim3((unsigned)(mtiles * a.ntiles_n)), dim3(C3T_THREADS), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// weight gradient in the Winograd form (conv3_wino_wgrad.h): h even, w a multiple of 32, everything below 2^31 bytes
bool conv3_wino_wgrad_takes(int n, int h, int w, int cin, int cout) {
    const int mode = conv3_wino_mode();
    if (mode == 0 || h % 2 != 0 || w % 2 != 0) return false;
    if ((long long)n * (h + 2) * (w + 2) * cin * 4 >= (1LL << 31) || (long long)n * h * w * cout * 4 >= (1LL << 31)) return false;
    return mode == 1 || (long long)n * (h / 2) * cdiv(w, 32) >= 512;
}

// xsaved != nullptr: the zero-bordered activated input already exists (written by ssdseg_conv3x3_fwd_saved), `in` is not read
int conv3_wino_wgrad_launch(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* dy, float* dw, int n, int h, int w, int cin, int cout,
                            const float* xsaved = nullptr) {
    WinoWgArgs a{};
    a.n = n; a.h = h; a.w = w; a.cin = cin; a.cout = cout;
    a.cpatches = cdiv(cin, WWG_KT); a.npatches = cdiv(cout, WWG_NT);
    a.strips = cdiv(w, 32);
    a.wrem = w - 32 * (a.strips - 1);
    a.steps = n * (h / 2) * a.strips;
    const int patches = a.cpatches * a.npatches;
    // one block per CU (100 KB of LDS, 8 waves): patches x steps units dealt evenly (WinoWgArgs); >= 4 steps per block
    long long span = ((long long)patches * a.steps + ctx->num_cus - 1) / ctx->num_cus;
    if (span < 4) span = 4;
    if (span > a.steps) span = a.steps;
    a.span = (int)span;
    a.full = a.steps / a.span;
    a.tail = a.steps - a.full * a.span;
    a.slots = a.full + (a.tail > 0 ? (a.tail + a.span - 1) / a.span + 1 : 0);
    const int nblocks = a.full * patches + (int)(((long long)patches * a.tail + a.span - 1) / a.span);
    const size_t xpb = xsaved != nullptr ? 0 : align256((size_t)n * (h + 2) * (w + 2) * cin * sizeof(float));
    const size_t pb = (size_t)patches * a.slots * 16 * WWG_KT * WWG_NT * sizeof(float);
    SSDSEG_ARG(pb < ((size_t)1 << 31), 9);
    void* ws;
    int rc = ssdseg_workspace(ctx, xpb + pb, &ws);
    if (rc) return rc;
    float* xp = (float*)ws;
    a.xp = xsaved != nullptr ? xsaved : xp; a.dy = dy; a.part = (float*)((char*)ws + xpb);
    a.xp_bytes = (unsigned)((size_t)n * (h + 2) * (w + 2) * cin * sizeof(float));
    a.dy_bytes = (unsigned)((size_t)n * h * w * cout * sizeof(float));
    a.part_bytes = (unsigned)pb;
    const double m = (double)n * h * w;
    if (xsaved == nullptr) {
        const long long tot4 = (long long)n * (h + 2) * (w + 2) * (cin / 4);
        SSDSEG_LAUNCH(ctx, 8.0 * m * cin, 0.0, conv3_pad_view_kernel, dim3((unsigned)((tot4 + 255) / 256 < 16384 ? (tot4 + 255) / 256 : 16384)), dim3(256), 0, in->x,
                      in->scale, in->shift, in->act, ldx, xp, n, h, w, cin, 0);
        SSDSEG_LAUNCH_CHECK();
    }
    if ((rc = conv3_announce_lds<&conv3_wino_wgrad_kernel>(WWG_LDS_BYTES))) return rc;
    const double cost_bytes = 4.0 * (m * cin + m * cout + 9.0 * cin * cout);   // X + dY + dW
    const double cost_flops = 8.0 * m * cin * cout;                             // executed MFMA flops: 16/36 of the direct form's 18 m cin cout
    SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, conv3_wino_wgrad_kernel, dim3((unsigned)nblocks), dim3(WWG_THREADS), WWG_LDS_BYTES, a);
    SSDSEG_LAUNCH_CHECK();
    const long long cn = (long long)cin * cout;
    SSDSEG_LAUNCH(ctx, 4.0 * cn * (16.0 * a.slots + 9.0), 0.0, conv3_wino_wgrad_finalize_kernel, dim3((unsigned)((cn + 255) / 256)), dim3(256), 0, (const float*)a.part, dw,
                  cin, cout, a.npatches, a.full, a.tail, a.span, a.slots);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
// split-K of a weight gradient over `steps` reduction steps: as many splits as `want` asks for while each keeps >= min_steps steps,
// dealt evenly (no empty split); returns the split count
template <typename T>
long long conv3_wgrad_splits(long long steps, long long want, int min_steps, T* steps_per_split) {
    long long splits = want;
    if (splits > steps / min_steps) splits = steps / min_steps;
    if (splits < 1) splits = 1;
    *steps_per_split = (T)((steps + splits - 1) / splits);
    return (steps + *steps_per_split - 1) / *steps_per_split;
}
// dw[9][cin][cout] from the `splits` partial slabs: fixed-order column sum (a copy when there is one slab)
int conv3_wgrad_reduce(ssdseg_ctx* ctx, const float* part, long long splits, int cin, int cout, float* dw) {
    if (splits == 1) {
        SSDSEG_HIP(hipMemcpyAsync(dw, part, (size_t)9 * cin * cout * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    return ssdseg_colsum(ctx, part, (int)splits, 9LL * cin * cout, dw);
}

}  // namespace

extern "C" {

int ssdseg_transpose_w(ssdseg_ctx* ctx, const float* w, float* wt, int cin, int cout, int taps) {
    SSDSEG_LAUNCH(ctx, 8.0 * taps * cin * cout, 0.0, conv3_transpose_w_kernel, dim3(cdiv(cout, 32), cdiv(cin, 32), taps), dim3(256), 0, w, wt, cin, cout);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ dense 3x3 (K6)
// partial rows of the BatchNorm statistics table each forward kernel writes (0 where it cannot take the layer, whatever the switches)
enum { C3_ROWA_K, C3_TILE_K, C3_WINO4_K };
static int conv3_fwd_rows(int n, int h, int w, int cin, int cout, int kind) {
    if (kind == C3_ROWA_K) return ssdseg_rowA_grid_y(n * h * w, cout);                      // implicit GEMM; tap-expanded (narrow) form
    if (cin % C3T_KC != 0) return 0;
    if (kind == C3_TILE_K) return conv3t_geometry(n, h, w, cout).mtiles;             // halo tiles, Winograd F(2x2): one row per 8 x 32 tile
    Wino4Geom g;                                                                      // F(4x4): one row per block of 4x4-pixel tiles
    return wino4_fits(h, w, cin, cout, &g) ? n * g.tiles_h * g.tiles_w : 0;
}

// rows the kernel that ssdseg_conv3x3_fwd / _fwd_saved_from launches under the current switches writes
static int conv3_fwd_rows_taken(int n, int h, int w, int ldx, int cin, int cout, bool saved) {
    if (!saved && (conv3_narrow(cin, cout) || !conv3_tile_fwd_ok(cin, cout) || !conv3_tile_fits(n, h, w, ldx)))
        return conv3_fwd_rows(n, h, w, cin, cout, C3_ROWA_K);
    // (halo tiles and Winograd F(2x2) share the tile grid; conv3_wino_launch hands over to F(4x4) where conv3_wino4_takes)
    return conv3_fwd_rows(n, h, w, cin, cout, conv3_wino4_takes(n, h, w, cin, cout) ? C3_WINO4_K : C3_TILE_K);
}

// the table is sized for the largest candidate (ssdseg_conv3x3_parts): zero the rows the launched kernel does not write
static int conv3_zero_unwritten_stats(ssdseg_ctx* ctx, float* stats, int n, int h, int w, int cin, int cout, int mine) {
    if (stats == nullptr) return 0;
    int nparts = 0;
    int rc = ssdseg_conv3x3_parts(n, h, w, cin, cout, &nparts);
    if (rc) return rc;
    if (nparts > mine) SSDSEG_HIP(hipMemsetAsync(stats + (size_t)mine * 2 * cout, 0, (size_t)(nparts - mine) * 2 * cout * sizeof(float), ctx->stream));
    return 0;
}

int ssdseg_conv3x3_parts(int n, int h, int w, int cin, int cout, int* nparts_host) {
    SSDSEG_ARG(n > 0 && h > 0 && w > 0, 1);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 4);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 5);
    SSDSEG_ARG(nparts_host != nullptr, 6);
    // sized for whichever forward kernel may run: the dispatch switches (SSDSEG_CONV3_*) are read again at launch time
    int rows = 0;
    for (int kind : {C3_ROWA_K, C3_TILE_K, C3_WINO4_K}) {
        const int r = conv3_fwd_rows(n, h, w, cin, cout, kind);
        if (r > rows) rows = r;
    }
    *nparts_host = rows;
    return 0;
}

int ssdseg_conv3x3_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int n, int h, int wdt, int cin,
                       int cout, float* stats) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= cin && ldx % 4 == 0, 3);
    SSDSEG_ARG(w != nullptr, 4);
    SSDSEG_ARG(y != nullptr, 5);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 6);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 9);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 10);
    if (conv3_narrow(cin, cout)) {
        Conv3nScratch s;
        int rc = conv3n_reserve(ctx, w, n, h, wdt, cin, cout, &s);
        if (rc) return rc;
        ctx->ws_reserved += s.bytes;
        rc = ssdseg_pwconv_fwd(ctx, in, ldx, s.w2, s.z, s.nc, (int)s.m, cin, s.nc, nullptr);
        ctx->ws_reserved -= s.bytes;
        if (rc) return rc;
        const int nparts = conv3_fwd_rows(n, h, wdt, cin, cout, C3_ROWA_K);
        SSDSEG_ARG((long long)s.m * s.cv < (1LL << 31), 6);   // 32-bit element indices in conv3n_tapsum_kernel
        rc = conv3_zero_unwritten_stats(ctx, stats, n, h, wdt, cin, cout, nparts);
        if (rc) return rc;
        int blocks = stats != nullptr ? nparts : (int)((s.m * s.cv + 255) / 256 < 4096 ? (s.m * s.cv + 255) / 256 : 4096);
        SSDSEG_LAUNCH(ctx, 4.0 * s.m * (s.nc + cout), 0.0, conv3n_tapsum_kernel, dim3(blocks), dim3(256), 0, (const float*)s.z, y, n, h, wdt, s.cv, stats);
        SSDSEG_LAUNCH_CHECK();
        return 0;
    }
    int rc = conv3_zero_unwritten_stats(ctx, stats, n, h, wdt, cin, cout, conv3_fwd_rows_taken(n, h, wdt, ldx, cin, cout, false));
    if (rc) return rc;
    if (conv3_tile_fwd_ok(cin, cout) && conv3_tile_fits(n, h, wdt, ldx)) {
        Conv3TArgs t = conv3t_args(in->x, in->scale, in->shift, in->act, ldx, y, cout, 0, stats, n, h, wdt, cin, cout);
        if (conv3_wino_takes(n, h, wdt, cin, cout)) return conv3_wino_launch(ctx, t, w, cin, cout, 0);
        // weights with the reduction channel contiguous: W[tap][c][n] -> Wt[tap][n][c] (2.8 MB for the decoder conv, ~3 us)
        void* ws;
        rc = ssdseg_workspace(ctx, (size_t)9 * cin * cout * sizeof(float), &ws);
        if (rc) return rc;
        rc = ssdseg_transpose_w(ctx, w, (float*)ws, cin, cout, 9);
        if (rc) return rc;
        t.wt = (const float*)ws;
        return conv3t_launch(ctx, t);
    }
    ssdseg_rowa_args a{};
    a.a0 = in->x; a.cs = in->scale; a.ct = in->shift; a.act = in->act; a.lda = ldx;
    a.b = w; a.ldb = cout;
    a.out = y; a.ldo = cout;
    a.stats = stats;
    a.I = n * h * wdt; a.R = 9 * cin; a.J = cout;
    a.convH = h; a.convW = wdt; a.convC = cin; a.convSign = 1;
    return ssdseg_rowA_conv3_fwd(ctx, a);
}

// ---- forward that SAVES its activated input for the weight gradient (large Winograd layers; include/ssdseg.h)
int ssdseg_conv3x3_saved_floats(int n, int h, int w, int cin, int cout, long long* floats_host) {
    SSDSEG_ARG(n > 0 && h > 0 && w > 0, 1);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 4);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 5);
    SSDSEG_ARG(floats_host != nullptr, 6);
    const bool both = !conv3_narrow(cin, cout) && getenv("SSDSEG_CONV3_WGRAD") == nullptr && getenv("SSDSEG_CONV3_SAVED") == nullptr &&
                      conv3_wino_takes(n, h, w, cin, cout) && conv3_wino_wgrad_takes(n, h, w, cin, cout);
    *floats_host = both ? (long long)n * (h + 2) * (w + 2) * cin : 0;
    return 0;
}

int ssdseg_conv3x3_fwd_saved(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int n, int h, int wdt, int cin, int cout,
                             float* stats, float* xsaved) {
    return ssdseg_conv3x3_fwd_saved_from(ctx, in, ldx, w, y, n, h, wdt, cin, cout, stats, xsaved, 0);
}

int ssdseg_conv3x3_fwd_saved_from(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int n, int h, int wdt, int cin,
                                  int cout, float* stats, float* xsaved, int c_from) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(c_from >= 0 && c_from < cin && c_from % 4 == 0, 13);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= cin && ldx % 4 == 0, 3);
    SSDSEG_ARG(w != nullptr, 4);
    SSDSEG_ARG(y != nullptr, 5);
    SSDSEG_ARG(xsaved != nullptr, 12);
    long long need = 0;
    int rc = ssdseg_conv3x3_saved_floats(n, h, wdt, cin, cout, &need);
    if (rc) return rc;
    SSDSEG_ARG(need > 0, 6);     // only for shapes ssdseg_conv3x3_saved_floats reports a size for
    rc = conv3_zero_unwritten_stats(ctx, stats, n, h, wdt, cin, cout, conv3_fwd_rows_taken(n, h, wdt, cin, cin, cout, true));
    if (rc) return rc;
    const long long tot4 = (long long)n * (h + 2) * (wdt + 2) * ((cin - c_from) / 4);
    SSDSEG_LAUNCH(ctx, 8.0 * n * h * wdt * (cin - c_from), 0.0, conv3_pad_view_kernel, dim3((unsigned)((tot4 + 255) / 256 < 16384 ? (tot4 + 255) / 256 : 16384)), dim3(256), 0,
                  in->x, in->scale, in->shift, in->act, ldx, xsaved, n, h, wdt, cin, c_from);
    SSDSEG_LAUNCH_CHECK();
    // (the input: pixel (1, 1) of image 0 of the zero-bordered copy)
    Conv3TArgs t = conv3t_args(xsaved + ((long long)(wdt + 2) + 1) * cin, nullptr, nullptr, SSDSEG_ACT_NONE, cin, y, cout, 0, stats, n, h, wdt, cin, cout);
    t.in_hp = h + 2; t.in_wp = wdt + 2;
    return conv3_wino_launch(ctx, t, w, cin, cout, 0);
}

int ssdseg_conv3x3_bwd_weight_saved(ssdseg_ctx* ctx, const float* xsaved, const float* dy, float* dw, int n, int h, int wdt, int cin, int cout) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(xsaved != nullptr, 2);
    SSDSEG_ARG(dy != nullptr, 3);
    SSDSEG_ARG(dw != nullptr, 4);
    long long need = 0;
    int rc = ssdseg_conv3x3_saved_floats(n, h, wdt, cin, cout, &need);
    if (rc) return rc;
    SSDSEG_ARG(need > 0, 5);
    return conv3_wino_wgrad_launch(ctx, nullptr, cin, dy, dw, n, h, wdt, cin, cout, xsaved);
}

// input gradient in the tap-expanded form: dz[m][tap][o] = dy[m - d(tap)][o], then dx = dz * W2^T is a pointwise GEMM.  in != nullptr:
// the GEMM's float4 epilogue holds the dx tile and reads the matching tile of the raw input -- that BN's sums ride there (the 256 -> 4
// logits conv of the decoder: one pass over the 614,400 x 256 gradient and its raw tensor less)
static int conv3n_bwd_data(ssdseg_ctx* ctx, const ssdseg_view* in, const ssdseg_gview* dy, const float* w, float* dx, int ldx, int n, int h, int wdt,
                           int cin, int cout, int accumulate, const float* in_mean, const float* in_invstd, float* in_dgamma, float* in_dbeta,
                           float* in_k1, float* in_k0) {
    Conv3nScratch s;
    int rc = conv3n_reserve(ctx, w, n, h, wdt, cin, cout, &s);
    if (rc) return rc;
    rc = conv3n_shift(ctx, dy, s, n, h, wdt, cout);
    if (rc) return rc;
    ssdseg_gview idv{};
    idv.g = s.z;
    ctx->ws_reserved += s.bytes;
    if (in != nullptr) rc = ssdseg_pwconv_bwd_data_bn(ctx, in, ldx, &idv, s.nc, s.w2, dx, ldx, (int)s.m, cin, s.nc, in_mean, in_invstd, in_dgamma, in_dbeta, in_k1, in_k0);
    else rc = ssdseg_pwconv_bwd_data(ctx, &idv, s.nc, s.w2, dx, ldx, (int)s.m, cin, s.nc, nullptr, 0, accumulate);
    ctx->ws_reserved -= s.bytes;
    return rc;
}

int ssdseg_conv3x3_bwd_data_bn(ssdseg_ctx* ctx, const ssdseg_view* in, const ssdseg_gview* dy, const float* w, float* dx, int ldx, int n,
                               int h, int wdt, int cin, int cout, const float* in_mean, const float* in_invstd, float* in_dgamma,
                               float* in_dbeta, float* in_k1, float* in_k0) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && in->scale != nullptr && in->shift != nullptr, 2);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 3);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 3);
    SSDSEG_ARG(w != nullptr, 4);
    SSDSEG_ARG(dx != nullptr, 5);
    SSDSEG_ARG(ldx >= cin && ldx % 4 == 0, 6);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 7);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 10);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 11);
    SSDSEG_ARG(in_mean != nullptr && in_invstd != nullptr, 12);
    SSDSEG_ARG(in_k1 != nullptr && in_k0 != nullptr, 16);
    const long long m = (long long)n * h * wdt;
    if (conv3_narrow(cin, cout) && ssdseg_conv3n_direct_takes(cin, cout, ldx) && m < (1LL << 29))      // conv3n.hip: the streaming form (256 -> 4)
        return ssdseg_conv3n_bwd_bn_direct(ctx, in, dy, w, dx, ldx, n, h, wdt, in_mean, in_invstd, in_dgamma, in_dbeta, in_k1, in_k0);
    if (conv3_narrow(cin, cout))
        return conv3n_bwd_data(ctx, in, dy, w, dx, ldx, n, h, wdt, cin, cout, 0, in_mean, in_invstd, in_dgamma, in_dbeta, in_k1, in_k0);
    int rc = ssdseg_conv3x3_bwd_data(ctx, dy, w, dx, ldx, n, h, wdt, cin, cout, 0);
    if (rc) return rc;
    return ssdseg_bn_bwd_reduce(ctx, dx, ldx, in->x, ldx, (int)m, cin, in->scale, in->shift, in_mean, in_invstd, in->act, in_dgamma, in_dbeta, in_k1, in_k0);
}

int ssdseg_conv3x3_bwd_data(ssdseg_ctx* ctx, const ssdseg_gview* dy, const float* w, float* dx, int ldx, int n, int h, int wdt,
                            int cin, int cout, int accumulate) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 2);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 2);
    SSDSEG_ARG(w != nullptr, 3);
    SSDSEG_ARG(dx != nullptr, 4);
    SSDSEG_ARG(ldx >= cin, 5);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 6);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 9);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 10);
    if (conv3_narrow(cin, cout))
        return conv3n_bwd_data(ctx, nullptr, dy, w, dx, ldx, n, h, wdt, cin, cout, accumulate, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (conv3_tile_enabled() && dy->scale == nullptr && cout % C3T_KC == 0 && conv3_tile_fits(n, h, wdt, cout)) {
        // dx[p][c] = sum_{tap, n} dy[p - d(tap)][n] W[tap][c][n]: the forward loop over the mirrored taps; W's native layout already has
        // the reduction channel (n) contiguous.  (A BatchNorm gradient view is materialised by the caller first: nine taps would
        // each re-form it -- ssdseg_gview_materialize.)
        Conv3TArgs t = conv3t_args(dy->g, nullptr, nullptr, SSDSEG_ACT_NONE, cout, dx, ldx, accumulate, nullptr, n, h, wdt, cout, cin);
        if (conv3_wino_takes(n, h, wdt, cout, cin)) return conv3_wino_launch(ctx, t, w, cin, cout, 1);
        t.wt = w;
        t.flip = 1;
        return conv3t_launch(ctx, t);
    }
    ssdseg_rowa_args a{};
    a.a0 = dy->g; a.a1 = dy->y; a.cs = dy->scale; a.ct = dy->shift; a.ck1 = dy->k1; a.ck0 = dy->k0; a.act = dy->act;
    a.lda = cout;
    a.b = w; a.ldb = cout;
    a.out = dx; a.ldo = ldx;
    a.accumulate = accumulate;
    a.I = n * h * wdt; a.R = 9 * cout; a.J = cin;
    a.convH = h; a.convW = wdt; a.convC = cout; a.convSign = -1;   // dx(h,w) gathers dy(h-(kh-1), w-(kw-1))
    return ssdseg_rowA_conv3_bwd_data(ctx, a);
}

int ssdseg_conv3x3_bwd_weight(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, float* dw, int n, int h,
                              int wdt, int cin, int cout) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= cin && ldx % 4 == 0, 3);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 4);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 4);
    SSDSEG_ARG(dw != nullptr, 5);
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 6);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 9);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 10);
    if (conv3_narrow(cin, cout)) {
        Conv3nScratch s;      // (s.w2 holds dW2 here)
        int rc = conv3n_reserve(ctx, nullptr, n, h, wdt, cin, cout, &s);
        if (rc) return rc;
        rc = conv3n_shift(ctx, dy, s, n, h, wdt, cout);
        if (rc) return rc;
        ssdseg_wgrad_args a{};
        a.x = in->x; a.xs = in->scale; a.xt = in->shift; a.xact = in->act; a.ldx = ldx;
        a.g = s.z; a.ldy = s.nc;
        a.M = (int)s.m; a.K = cin; a.N = s.nc;
        ctx->ws_reserved += s.bytes;
        ssdseg_defer_hold(ctx, +1);           // dW2 is scratch, repacked right below: its column sum cannot wait for the flush
        rc = ssdseg_wgrad_run(ctx, a, s.w2);
        ssdseg_defer_hold(ctx, -1);
        ctx->ws_reserved -= s.bytes;
        if (rc) return rc;
        SSDSEG_LAUNCH(ctx, 8.0 * 9 * cin * cout, 0.0, conv3n_pack_w_kernel, dim3(cdiv(9 * cin * cout, 256)), dim3(256), 0, (const float*)dw, s.w2, cin, cout, 1);
        SSDSEG_LAUNCH_CHECK();
        return 0;
    }
    // "taps": the nine shifted GEMMs, "nine": the nine-wave kernel for every tile width (A/B measurements, parity tests)
    const char* c3env = getenv("SSDSEG_CONV3_WGRAD");
    if (c3env == nullptr && dy->scale == nullptr && conv3_wino_wgrad_takes(n, h, wdt, cin, cout))
        return conv3_wino_wgrad_launch(ctx, in, ldx, dy->g, dw, n, h, wdt, cin, cout);
    if (c3env == nullptr && conv3_tile_enabled() && dy->scale == nullptr && conv3_tile_fits(n, h, wdt, ldx) && conv3_tile_fits(n, h, wdt, cout)) {
        // halo-tile form (conv3_wgrad_tile.h): 64 x 64 (k, n) tiles of all nine taps, one image row x 32 columns per step
        Wg3TArgs a{};
        a.x = in->x; a.xs = in->scale; a.xt = in->shift; a.xact = in->act; a.ldx = ldx;
        a.g = dy->g;
        a.n = n; a.h = h; a.w = wdt; a.K = cin; a.N = cout;
        a.ktiles = cdiv(cin, W3T_KT); a.ntiles = cdiv(cout, W3T_NT);
        a.strips = cdiv(wdt, W3T_COLS);
        a.steps = n * a.strips * h;
        const int tiles = a.ktiles * a.ntiles;
        const long long splits = conv3_wgrad_splits(a.steps, 2 * ctx->num_cus / tiles, 4, &a.steps_per_split);   // two blocks per CU (67 KB of LDS, <= 256 registers each)
        a.x_bytes = (unsigned)((((long long)n * h * wdt - 1) * ldx + cin) * 4);
        a.g_bytes = (unsigned)((long long)n * h * wdt * cout * 4);
        void* ws;
        int rc = ssdseg_partials(ctx, (size_t)splits * 9 * cin * cout * sizeof(float), &ws);
        if (rc) return rc;
        a.part = (float*)ws;
        if ((rc = conv3_announce_lds<&conv3_wgrad_tile_kernel>(W3T_LDS_BYTES))) return rc;
        const double m = (double)n * h * wdt;
        const double cost_bytes = 4.0 * (m * cin + m * cout + 9.0 * cin * cout);   // X + dY + dW
        const double cost_flops = 18.0 * m * cin * cout;
        SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, conv3_wgrad_tile_kernel, dim3((unsigned)(tiles * splits)), dim3(W3T_THREADS), W3T_LDS_BYTES, a);
        SSDSEG_LAUNCH_CHECK();
        return conv3_wgrad_reduce(ctx, a.part, splits, cin, cout, dw);
    }
    if (!(c3env != nullptr && !strcmp(c3env, "taps"))) {
        // all nine taps in one pass (conv3_wgrad.h)
        Conv9Args a{};
        a.x = in->x; a.xs = in->scale; a.xt = in->shift; a.xact = in->act; a.ldx = ldx;
        a.g = dy->g; a.y = dy->y; a.gs = dy->scale; a.gt = dy->shift; a.gk1 = dy->k1; a.gk0 = dy->k0; a.gact = dy->act;
        a.n = n; a.h = h; a.w = wdt; a.K = cin; a.N = cout;
        a.wchunks = cdiv(wdt, C9_PX);
        a.steps = (long long)n * h * a.wchunks;
        const int wn = cout > 32 ? 4 : 1;
        const int gx = cdiv(cout, 32 * wn), gy = cdiv(cin, C9_KT);
        const long long splits = conv3_wgrad_splits(a.steps, (2LL * ctx->num_cus) / ((long long)gx * gy), 8, &a.steps_per_split);
        void* ws;
        int rc = ssdseg_partials(ctx, (size_t)splits * 9 * cin * cout * sizeof(float), &ws);
        if (rc) return rc;
        a.part = (float*)ws;
        const dim3 grid(gx, gy, (unsigned)splits);
        const size_t lds = (size_t)(C9_PX * (32 * wn + 4) + 3 * C9_XW * C9_XS) * sizeof(float);
        const double m = (double)n * h * wdt;
        const double cost_bytes = 4.0 * (m * cin + m * cout + 9.0 * cin * cout);   // 8(d): X + dY + dW
        ctx->timing_view_bytes = dy->scale != nullptr ? 4.0 * m * cout : 0.0;
        const double cost_flops = 18.0 * m * cin * cout;
        if (wn == 4 && !(c3env != nullptr && !strcmp(c3env, "nine")))
            SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, conv3_wgrad12_kernel, grid, dim3(C12_THREADS), lds, a);
        else if (wn == 4) SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, (conv3_wgrad9_kernel<4>), grid, dim3(C9_THREADS), lds, a);
        else SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, (conv3_wgrad9_kernel<1>), grid, dim3(C9_THREADS), lds, a);
        SSDSEG_LAUNCH_CHECK();
        return conv3_wgrad_reduce(ctx, a.part, splits, cin, cout, dw);
    }
    for (int tap = 0; tap < 9; ++tap) {
        ssdseg_wgrad_args a{};
        a.x = in->x; a.xs = in->scale; a.xt = in->shift; a.xact = in->act; a.ldx = ldx;
        a.g = dy->g; a.y = dy->y; a.gs = dy->scale; a.gt = dy->shift; a.gk1 = dy->k1; a.gk0 = dy->k0; a.gact = dy->act;
        a.ldy = cout;
        a.M = n * h * wdt; a.K = cin; a.N = cout;
        a.convH = h; a.convW = wdt; a.dh = tap / 3 - 1; a.dw = tap % 3 - 1;
        int rc = ssdseg_wgrad_run(ctx, a, dw + (size_t)tap * cin * cout);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
