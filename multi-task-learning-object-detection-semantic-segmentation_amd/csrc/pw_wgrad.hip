// Weight gradient of the pointwise (1x1) convolutions and of everything lowered onto them (dense 3x3 taps, the stem):
//   dw[k][n] = sum_m a[m][k] * dy[m][n]      split over m, fixed-order reduce
// Two kernels: the row-naming form (pw_wgrad.h) for plain aligned operands, gemm_wgrad_kernel for the rest.
#include "gemm_internal.h"

namespace {

struct WGradArgs : ssdseg_wgrad_args {};

// reduction rows per wave per step: 64 rows per block step when the waves split the rows 4- or 2-way, 32 when all four waves
// sit along k (16-row steps left that shape with two barriers per 8 MFMAs: 2.5-3.2 TB/s of real traffic)
constexpr int rw_of(int wr) { return wr == 4 ? 16 : 32; }

// WI waves along the output rows (k), WR waves splitting the reduction rows (m); WI*WR == 4.
// occupancy targets where the raw-load staging would otherwise cost a wave per SIMD (184 registers for <4,1,3>: 2 waves instead of 3)
constexpr int wgrad_min_waves(int WI, int WR, int WN) { return (WI == 4 && WN <= 2) ? 3 : 1; }
template <int WI, int WR, int WN>
__global__ void __launch_bounds__(256, wgrad_min_waves(WI, WR, WN)) gemm_wgrad_kernel(WGradArgs p) {
    constexpr int RW = rw_of(WR);
    constexpr int BI = 32 * WI, BJ = 32 * WN, BRT = RW * WR;
    extern __shared__ float smem[];
    float* Xs = smem;              // [BRT][BI]
    float* Ys = smem + BRT * BI;   // [BRT][BJ]
    const int t = threadIdx.x;
    const int wave = t >> 6, lane = t & 63, li = lane & 31, hh = lane >> 5;
    const int wi = wave % WI, wr = wave / WI;
    const int i0 = blockIdx.y * BI;   // k offset
    const int j0 = blockIdx.x * BJ;   // n offset
    const int split = blockIdx.z;
    const long long mbeg = (long long)split * p.rows_per_split;
    long long mend = mbeg + p.rows_per_split;
    if (mend > p.M) mend = p.M;
    const bool xaff = p.xs != nullptr, gaff = p.gs != nullptr;
    const float xlo = act_lo(p.xact), xhi = act_hi(p.xact);
    const float* yptr = gaff ? p.y : p.g;                        // identity gradient view: y aliases g, act NONE
    const int yact = gaff ? p.gact : SSDSEG_ACT_NONE;

    constexpr int XV = BRT * BI / 4;   // float4 per X tile (== 256 * 2)
    constexpr int YV = BRT * BJ / 4;
    constexpr int XQ = (XV + 255) / 256, YQ = (YV + 255) / 256;
    // Staging in two halves (as in gemm_wres.h): load_tiles() only issues the RAW loads of the next step; store_tiles() -- one
    // MFMA phase and a barrier later -- applies the views and writes LDS.  With the view arithmetic inside load_tiles every
    // step waited for its global loads before the first MFMA.  The per-channel view coefficients sit in LDS (loaded once).
    // (RAW = false: the 96-column tiles of the 30x40 / 15x20 stages, where the extra staging registers cost a wave per SIMD)
    constexpr bool RAW = !(WI == 4 && WN == 3);
    float4 xraw[RAW ? XQ : 1], graw[RAW ? YQ : 1], yraw[RAW ? YQ : 1];
    unsigned xok = 0, yok = 0;   // bit q (stem: bit 4q + element): the slot holds real data
    float* Xc = smem + BRT * (BI + BJ);   // [2][BI]: scale, shift of the X view
    float* Yc = Xc + 2 * BI;              // [4][BJ]: scale, shift, k1, k0 of the gradient view
    for (int i = t; i < BI; i += 256) {
        const int k = i0 + i;
        const bool ok = xaff && k < p.K;
        Xc[i] = ok ? p.xs[k] : 1.f;
        Xc[BI + i] = ok ? p.xt[k] : 0.f;
    }
    for (int i = t; i < BJ; i += 256) {
        const int n = j0 + i;
        const bool ok = gaff && n < p.N;
        Yc[i] = ok ? p.gs[n] : 1.f;
        Yc[BJ + i] = ok ? p.gt[n] : 0.f;
        Yc[2 * BJ + i] = ok ? p.gk1[n] : 0.f;
        Yc[3 * BJ + i] = ok ? p.gk0[n] : 0.f;
    }
    // (made visible by the first barrier of the main loop)

    auto load_tiles = [&](long long mrow) {
        xok = yok = 0;
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = t + 256 * q;
            float4 v = f4(0.f);
            if (idx < XV) {
                const int rr = idx / (BI / 4), c4 = idx % (BI / 4);
                const long long m = mrow + rr;
                const int k = i0 + c4 * 4;
                bool ok = m < mend && k < p.K;
                long long src = m;
                if (p.stem) {
                    const long long hw = (long long)p.convH * p.convW;
                    const long long img = m / hw;
                    const int rem = (int)(m - img * hw);
                    const int ho = rem / p.convW, wo = rem - ho * p.convW;
                    float e[4];
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int rq = k + qq, tap = rq / 3, ci = rq - tap * 3, kh = tap / 3, kw = tap - kh * 3;
                        const int hi = 2 * ho + kh - p.stemPt, wi = 2 * wo + kw - p.stemPl;
                        const bool okq = m < mend && rq < p.K && hi >= 0 && hi < p.stemH && wi >= 0 && wi < p.stemW;
                        e[qq] = p.x[okq ? ((img * p.stemH + hi) * p.stemW + wi) * 3 + ci : 0];
                        xok |= (okq ? 1u : 0u) << (4 * q + qq);
                    }
                    xraw[q] = make_float4(e[0], e[1], e[2], e[3]);
                    continue;
                }
                if (p.convH > 0 && ok) {
                    const long long hw = (long long)p.convH * p.convW;
                    const long long img = m / hw;
                    const int rem = (int)(m - img * hw);
                    const int hy = rem / p.convW + p.dh, wx = rem % p.convW + p.dw;
                    ok = hy >= 0 && hy < p.convH && wx >= 0 && wx < p.convW;
                    src = (img * p.convH + hy) * p.convW + wx;
                }
                v = ld4(p.x + (ok ? src * p.ldx + k : 0));
                xok |= (ok ? 1u : 0u) << (p.stem ? 4 * q : q);
            }
            xraw[q] = v;
        }
#pragma unroll
        for (int q = 0; q < YQ; ++q) {
            const int idx = t + 256 * q;
            float4 g4 = f4(0.f), y4 = f4(0.f);
            if (idx < YV) {
                const int rr = idx / (BJ / 4), c4 = idx % (BJ / 4);
                const long long m = mrow + rr;
                const int n = j0 + c4 * 4;
                const bool ok = m < mend && n < p.N;
                const long long o = ok ? m * p.ldy + n : 0;
                g4 = ld4(p.g + o);
                y4 = ld4(yptr + o);
                yok |= (ok ? 1u : 0u) << q;
            }
            graw[q] = g4;
            yraw[q] = y4;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = t + 256 * q;
            if (idx < XV) {
                const int c4 = idx % (BI / 4);
                float4 v;
                if (p.stem) {
                    v.x = ((xok >> (4 * q + 0)) & 1u) ? fmaf(xraw[q].x, p.stemScale, p.stemOffset) : 0.f;
                    v.y = ((xok >> (4 * q + 1)) & 1u) ? fmaf(xraw[q].y, p.stemScale, p.stemOffset) : 0.f;
                    v.z = ((xok >> (4 * q + 2)) & 1u) ? fmaf(xraw[q].z, p.stemScale, p.stemOffset) : 0.f;
                    v.w = ((xok >> (4 * q + 3)) & 1u) ? fmaf(xraw[q].w, p.stemScale, p.stemOffset) : 0.f;
                } else {
                    v = view_affine4(xraw[q], ld4(Xc + c4 * 4), ld4(Xc + BI + c4 * 4), xlo, xhi);
                    if (!((xok >> q) & 1u)) v = f4(0.f);
                }
                st4(Xs + idx * 4, v);
            }
        }
#pragma unroll
        for (int q = 0; q < YQ; ++q) {
            const int idx = t + 256 * q;
            if (idx < YV) {
                const int c4 = idx % (BJ / 4);
                float4 v = gview_apply4(graw[q], yraw[q], ld4(Yc + c4 * 4), ld4(Yc + BJ + c4 * 4), ld4(Yc + 2 * BJ + c4 * 4),
                                        ld4(Yc + 3 * BJ + c4 * 4), yact);
                if (!((yok >> q) & 1u)) v = f4(0.f);
                st4(Ys + idx * 4, v);
            }
        }
    };

    // ---- the original staging (view arithmetic at load time), kept for the shapes where it measured faster
    float4 xreg[RAW ? 1 : XQ], yreg[RAW ? 1 : YQ];   // !RAW: transformed at load time

    // per-thread channel coefficients are fixed across steps when the tile width divides 256 float4 columns;
    // otherwise they are re-read per step (they sit in L1).
    auto load_tiles_t = [&](long long mrow) {
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = t + 256 * q;
            float4 v = f4(0.f);
            if (idx < XV) {
                const int rr = idx / (BI / 4), c4 = idx % (BI / 4);
                const long long m = mrow + rr;
                const int k = i0 + c4 * 4;
                bool ok = m < mend && k < p.K;
                long long src = m;
                if (p.stem) {
                    const long long hw = (long long)p.convH * p.convW;
                    const long long img = m / hw;
                    const int rem = (int)(m - img * hw);
                    const int ho = rem / p.convW, wo = rem - ho * p.convW;
                    float e[4];
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int rq = k + qq, tap = rq / 3, ci = rq - tap * 3, kh = tap / 3, kw = tap - kh * 3;
                        const int hi = 2 * ho + kh - p.stemPt, wi = 2 * wo + kw - p.stemPl;
                        const bool okq = m < mend && rq < p.K && hi >= 0 && hi < p.stemH && wi >= 0 && wi < p.stemW;
                        const float xv = p.x[okq ? ((img * p.stemH + hi) * p.stemW + wi) * 3 + ci : 0];
                        e[qq] = okq ? fmaf(xv, p.stemScale, p.stemOffset) : 0.f;
                    }
                    xreg[q] = make_float4(e[0], e[1], e[2], e[3]);
                    continue;
                }
                if (p.convH > 0 && ok) {
                    const long long hw = (long long)p.convH * p.convW;
                    const long long img = m / hw;
                    const int rem = (int)(m - img * hw);
                    const int hy = rem / p.convW + p.dh, wx = rem % p.convW + p.dw;
                    ok = hy >= 0 && hy < p.convH && wx >= 0 && wx < p.convW;
                    src = (img * p.convH + hy) * p.convW + wx;
                }
                {
                    const int kk = ok ? k : 0;
                    float4 s = f4(1.f), sh = f4(0.f);
                    if (xaff) { s = ld4(p.xs + kk); sh = ld4(p.xt + kk); }
                    v = view_affine4(ld4(p.x + (ok ? src * p.ldx + k : 0)), s, sh, xlo, xhi);
                    if (!ok) v = f4(0.f);
                }
            }
            xreg[q] = v;
        }
#pragma unroll
        for (int q = 0; q < YQ; ++q) {
            const int idx = t + 256 * q;
            float4 v = f4(0.f);
            if (idx < YV) {
                const int rr = idx / (BJ / 4), c4 = idx % (BJ / 4);
                const long long m = mrow + rr;
                const int n = j0 + c4 * 4;
                {
                    const bool ok = m < mend && n < p.N;
                    const long long o = ok ? m * p.ldy + n : 0;
                    const int nn = ok ? n : 0;
                    float4 gs = f4(1.f), gt = f4(0.f), gk1 = f4(0.f), gk0 = f4(0.f);
                    if (gaff) { gs = ld4(p.gs + nn); gt = ld4(p.gt + nn); gk1 = ld4(p.gk1 + nn); gk0 = ld4(p.gk0 + nn); }
                    v = gview_apply4(ld4(p.g + o), ld4(yptr + o), gs, gt, gk1, gk0, yact);
                    if (!ok) v = f4(0.f);
                }
            }
            yreg[q] = v;
        }
    };
    auto store_tiles_t = [&]() {
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int idx = t + 256 * q;
            if (idx < XV) st4(Xs + idx * 4, xreg[q]);
        }
#pragma unroll
        for (int q = 0; q < YQ; ++q) {
            const int idx = t + 256 * q;
            if (idx < YV) st4(Ys + idx * 4, yreg[q]);
        }
    };


    f32x16 acc[WN];
#pragma unroll
    for (int nt = 0; nt < WN; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;

    if (mbeg < mend) { if (RAW) load_tiles(mbeg); else load_tiles_t(mbeg); }
    for (long long mrow = mbeg; mrow < mend; mrow += BRT) {
        __syncthreads();
        if (RAW) store_tiles(); else store_tiles_t();
        __syncthreads();
        if (mrow + BRT < mend) { if (RAW) load_tiles(mrow + BRT); else load_tiles_t(mrow + BRT); }
        const float* xa = Xs + (wr * RW + hh) * BI + wi * 32 + li;
        const float* yb = Ys + (wr * RW + hh) * BJ + li;
        // fragments of step st + 2 are read while the MFMAs of step st run (see gemm_rowA_kernel: no per-MFMA LDS round trip)
        constexpr int PF = 2, NST = RW / 2;
        float afr[PF + 1], bfr[PF + 1][WN];
        auto fetch = [&](int st, int buf) {
            afr[buf] = xa[(2 * st) * BI];
#pragma unroll
            for (int nt = 0; nt < WN; ++nt) bfr[buf][nt] = yb[(2 * st) * BJ + nt * 32];
        };
#pragma unroll
        for (int q = 0; q < PF; ++q) fetch(q, q);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            if (st + PF < NST) fetch(st + PF, (st + PF) % (PF + 1));
            __builtin_amdgcn_sched_barrier(0);   // keep those reads in front of this step's MFMAs
#pragma unroll
            for (int nt = 0; nt < WN; ++nt) acc[nt] = mfma32(afr[st % (PF + 1)], bfr[st % (PF + 1)][nt], acc[nt]);
        }
    }

    // reduce the WR reduction-waves through LDS, then write the split's partial tile
    float* out = p.part + (long long)split * p.K * p.N;
    if (WR > 1) {
        __syncthreads();
        float* red = smem;  // [WR-1][WI][WN][16][64]
        if (wr > 0) {
#pragma unroll
            for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                for (int e = 0; e < 16; ++e) red[((((wr - 1) * WI + wi) * WN + nt) * 16 + e) * 64 + lane] = acc[nt][e];
        }
        __syncthreads();
        if (wr == 0) {
#pragma unroll
            for (int q = 1; q < WR; ++q)
#pragma unroll
                for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[nt][e] += red[((((q - 1) * WI + wi) * WN + nt) * 16 + e) * 64 + lane];
        }
    }
    if (wr == 0) {
#pragma unroll
        for (int nt = 0; nt < WN; ++nt) {
            const int n = j0 + nt * 32 + li;
            if (n < p.N) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = i0 + wi * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                    if (k < p.K) out[(long long)k * p.N + n] = acc[nt][e];
                }
            }
        }
    }
}

#include "pw_wgrad.h"

// 8(d): read X, read dY, write dW; the raw y of a BatchNorm-backward gradient view is reported as `view_bytes`
struct WGradCost { double bytes, flops; };
WGradCost wgrad_cost(ssdseg_ctx* ctx, int M, int K, int N, bool gview) {
    ctx->timing_view_bytes = gview ? 4.0 * M * N : 0.0;
    return {4.0 * ((double)M * K + (double)M * N + (double)K * N), 2.0 * M * K * N};
}

template <int WI, int WR, int WN>
int launch_wgrad(ssdseg_ctx* ctx, const WGradArgs& a, dim3 grid) {
    constexpr size_t tiles = ((size_t)(rw_of(WR) * WR) * (32 * WI + 32 * WN) + 2 * 32 * WI + 4 * 32 * WN) * sizeof(float);   // tiles + view coefficients
    constexpr size_t red = (size_t)(WR - 1) * WI * WN * 16 * 64 * sizeof(float);
    constexpr size_t lds = red > tiles ? red : tiles;
    const WGradCost c = wgrad_cost(ctx, a.M, a.K, a.N, a.gs != nullptr);
    char kbuf[64];
    snprintf(kbuf, sizeof(kbuf), "gemm_wgrad_kernel<%d, %d, %d>%s", WI, WR, WN, a.convH > 0 ? " [conv3x3 tap]" : "");
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    SSDSEG_LAUNCH_NAMED(ctx, kname, c.bytes, c.flops, (gemm_wgrad_kernel<WI, WR, WN>), grid, dim3(256), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// partial slabs of a split weight gradient (splits * K * N floats, written once and read once by the column sum) are kept below this
// fraction of the layer's operand traffic M * (K + N)  (SSDSEG_WGRAD_SLAB_FRAC, read per call: A/B runs)
double slab_fraction() {
    const char* e = getenv("SSDSEG_WGRAD_SLAB_FRAC");   // (a fraction: not one of the env_is / env_int switches)
    const double f = e != nullptr ? atof(e) : 0.5;
    return f > 0.0 ? f : 0.5;
}

// ---- pointwise weight gradient, row-naming form (pw_wgrad.h).  SSDSEG_PW_WGRAD=0: gemm_wgrad_kernel for everything.
template <int JX, int JY, int WK, int WN>
int pw_wgrad_launch(ssdseg_ctx* ctx, PwWgArgs a, float* dw) {
    constexpr int G = 8 / (WK * WN), KT = 32 * JX * WK, NT = 32 * JY * WN, MS = pww_ms(KT, NT);
    const int ktiles = cdiv(a.K, KT), ntiles = cdiv(a.N, NT);
    const long long steps = ((long long)a.M + MS - 1) / MS;
    // blocks: two per CU; every split >= 4 steps; partial slabs (splits * K * N, written and re-read) below half the operand traffic
    long long splits = (2LL * ctx->num_cus + (long long)ktiles * ntiles - 1) / ((long long)ktiles * ntiles);
    const long long cap_steps = (steps + 3) / 4;
    const long long cap_traffic = (long long)((double)a.M * (a.K + a.N) * slab_fraction() / ((double)a.K * a.N));
    if (splits > cap_steps) splits = cap_steps;
    if (splits > cap_traffic) splits = cap_traffic;
    if (splits < 1) splits = 1;
    if (splits > 65535) splits = 65535;
    const long long sps = (steps + splits - 1) / splits;
    splits = (steps + sps - 1) / sps;
    a.rows_per_split = (int)(sps * MS);
    const long long slabs = splits;
    const size_t pb = (size_t)slabs * a.K * a.N * sizeof(float);
    if (pb >= ((size_t)1 << 31)) return -1;
    float* part = dw;
    if (slabs > 1) {
        void* ws;
        int rc = ssdseg_partials(ctx, pb, &ws);
        if (rc) return rc;
        part = (float*)ws;
    }
    a.part = part;
    a.part_bytes = (unsigned)pb;
    const size_t lds = pww_lds_bytes(KT, NT, G);
    static bool configured = false;      // (per instantiation) dynamic LDS beyond 64 KiB has to be announced once
    if (lds > 64 * 1024 && !configured) {
        SSDSEG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_wgrad_kernel<JX, JY, WK, WN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        configured = true;
    }
    const WGradCost c = wgrad_cost(ctx, a.M, a.K, a.N, a.gs != nullptr);
    char kbuf[64];
    snprintf(kbuf, sizeof(kbuf), "pw_wgrad_kernel<%d, %d, %d, %d>", JX, JY, WK, WN);
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    SSDSEG_LAUNCH_NAMED(ctx, kname, c.bytes, c.flops, (pw_wgrad_kernel<JX, JY, WK, WN>), dim3(ntiles, ktiles, (unsigned)splits), dim3(512), lds, a);
    SSDSEG_LAUNCH_CHECK();
    if (slabs > 1) return ssdseg_colsum(ctx, part, (int)slabs, (long long)a.K * a.N, dw);
    return 0;
}

bool pw_wgrad_enabled() { return !env_is("SSDSEG_PW_WGRAD", '0'); }

// -> 0 launched, < 0 not taken (the caller falls back), > 0 error
int pw_wgrad_try(ssdseg_ctx* ctx, const WGradArgs& w, float* dw) {
    if (!pw_wgrad_enabled() || w.stem || w.convH > 0 || w.K % 4 != 0 || w.N % 4 != 0 || w.ldx % 4 != 0 || w.ldy % 4 != 0) return -1;
    // the pipelined issue() prefetches one step (<= 64 rows) past the end of a split and forms m0 * ld * 4 in 32 bits
    if (((long long)w.M + 64) * w.ldx * 4 >= (1LL << 31) || ((long long)w.M + 64) * w.ldy * 4 >= (1LL << 31)) return -1;
    PwWgArgs a{};
    a.x = w.x; a.xs = w.xs; a.xt = w.xt; a.xact = w.xact; a.ldx = w.ldx;
    a.g = w.g; a.y = w.y; a.gs = w.gs; a.gt = w.gt; a.gk1 = w.gk1; a.gk0 = w.gk0; a.gact = w.gact; a.ldy = w.ldy;
    a.M = w.M; a.K = w.K; a.N = w.N;
    a.x_bytes = (unsigned)((((long long)w.M - 1) * w.ldx + w.K) * 4);
    a.g_bytes = (unsigned)((((long long)w.M - 1) * w.ldy + w.N) * 4);
    // tile = (32 JX WK) x (32 JY WN), chosen per layer among the instantiated shapes (K = 160 on a 256-row tile wastes 37 % of the
    // MFMAs, three 64-row tiles 17 %; a 24 -> 144 layer on 64-column tiles reads x three times)
    struct Shape { int kt, nt; int (*launch)(ssdseg_ctx*, PwWgArgs, float*); };
    static const Shape shapes[] = {
        {256, 128, &pw_wgrad_launch<2, 2, 4, 2>}, {128, 256, &pw_wgrad_launch<2, 2, 2, 4>}, {128, 128, &pw_wgrad_launch<2, 2, 2, 2>},
        {256, 64, &pw_wgrad_launch<2, 2, 4, 1>},  {64, 128, &pw_wgrad_launch<2, 2, 1, 2>},  {128, 64, &pw_wgrad_launch<2, 2, 2, 1>},
        {256, 32, &pw_wgrad_launch<4, 1, 2, 1>},  {64, 64, &pw_wgrad_launch<2, 2, 1, 1>},   {32, 128, &pw_wgrad_launch<1, 4, 1, 1>},
        {128, 32, &pw_wgrad_launch<4, 1, 1, 1>},  {32, 64, &pw_wgrad_launch<1, 2, 1, 1>},   {64, 32, &pw_wgrad_launch<2, 1, 1, 1>},
        {32, 32, &pw_wgrad_launch<1, 1, 1, 1>}};
    // estimated time of a shape = max(padded MFMA work at ~110 TFLOP/s, operand traffic at ~4.5 TB/s): every n-tile re-reads the x
    // columns of its k-tile and vice versa, so small tiles cost traffic and large ones padding
    const Shape* best = nullptr;
    double best_t = 0.0;
    for (const Shape& sh : shapes) {
        const double tk = cdiv(w.K, sh.kt), tn = cdiv(w.N, sh.nt);
        const double t_mfma = 2.0 * w.M * (tk * sh.kt) * (tn * sh.nt) / 110e12;
        const double t_hbm = 4.0 * w.M * ((double)w.K * tn + (double)w.N * tk) / 4.5e12;
        const double t = t_mfma > t_hbm ? t_mfma : t_hbm;
        if (best == nullptr || t < best_t * 0.999) { best = &sh; best_t = t; }      // (listed largest first: ties keep the larger tile)
    }
    return best->launch(ctx, a, dw);
}

// picks the tile shape / split count for dw[k][n] = sum_m x[m][k]*dy[m][n], launches, reduces the split partials
int wgrad_run(ssdseg_ctx* ctx, WGradArgs a, float* dw) {
    {
        const int rc = pw_wgrad_try(ctx, a, dw);
        if (rc >= 0) return rc;
    }
    const int m = a.M, k = a.K, n = a.N;
    const int wi = k <= 32 ? 1 : (k <= 64 ? 2 : 4);
    const int wr = 4 / wi;
    const int brt = rw_of(wr) * wr;
    const int itiles = cdiv(k, 32 * wi);
    long long steps = ((long long)m + brt - 1) / brt;
    // split the reduction rows so that (a) the chip is full, (b) every block still does >= 4 steps and (c) the partial
    // slabs (splits*k*n floats, written then re-read) stay below half of the operand traffic m*(k+n)
    long long max_splits = (steps + 3) / 4;
    const long long traffic_cap = (long long)((double)m * (k + n) * slab_fraction() / ((double)k * n));
    if (max_splits > traffic_cap) max_splits = traffic_cap < 1 ? 1 : traffic_cap;
    int wn = pick_wn(n, (long long)itiles * max_splits);
    // the 4-way row-split shape stages 64 x (32*wn) of (g, y) per step: beyond 3 column tiles it needs > 256 VGPRs (1 wave/SIMD)
    if (wi == 1 && wn > 3) wn = 3;
    const int jtiles = cdiv(n, 32 * wn);
    // target blocks per CU: the long-M (HBM-bound) layers want more, shorter splits in flight; the short-M ones fewer, longer
    // splits (half the partial slabs, prologue / epilogue amortised over more steps)
    const long long bpc = m >= ROWA_OCC_ROWS ? env_int("SSDSEG_WGRAD_BPC_LONG", 4) : env_int("SSDSEG_WGRAD_BPC", 2);
    long long want = (bpc * ctx->num_cus + (long long)itiles * jtiles - 1) / ((long long)itiles * jtiles);
    long long splits = want < 1 ? 1 : (want > max_splits ? max_splits : want);
    if (splits > 65535) splits = 65535;
    long long steps_per_split = (steps + splits - 1) / splits;
    splits = (steps + steps_per_split - 1) / steps_per_split;
    a.rows_per_split = (int)(steps_per_split * brt);
    float* part = dw;
    if (splits > 1) {
        void* ws;
        int rc = ssdseg_partials(ctx, (size_t)splits * k * n * sizeof(float), &ws);
        if (rc) return rc;
        part = (float*)ws;
    }
    a.part = part;
    const dim3 grid(jtiles, itiles, (unsigned)splits);
    const int rc = for_width<1, 5>(wn, [&](auto W) {
        constexpr int WN = decltype(W)::value;
        if (wi == 1) return launch_wgrad<1, 4, WN>(ctx, a, grid);
        if (wi == 2) return launch_wgrad<2, 2, WN>(ctx, a, grid);
        return launch_wgrad<4, 1, WN>(ctx, a, grid);
    });
    if (rc) return rc;
    if (splits > 1) return ssdseg_colsum(ctx, part, (int)splits, (long long)k * n, dw);
    return 0;
}

}  // namespace

extern "C" {

int ssdseg_wgrad_run(ssdseg_ctx* ctx, const ssdseg_wgrad_args& a, float* dw) { return wgrad_run(ctx, WGradArgs{a}, dw); }

int ssdseg_pwconv_bwd_weight(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy, float* dw,
                             int m, int k, int n) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= k && ldx % 4 == 0, 3);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 4);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 4);
    SSDSEG_ARG(ldy >= n && ldy % 4 == 0, 5);
    SSDSEG_ARG(dw != nullptr, 6);
    SSDSEG_ARG(m > 0, 7);
    SSDSEG_ARG(k > 0 && k % 4 == 0, 8);
    SSDSEG_ARG(n > 0 && n % 4 == 0, 9);
    WGradArgs a{};
    a.x = in->x; a.xs = in->scale; a.xt = in->shift; a.xact = in->act; a.ldx = ldx;
    a.g = dy->g; a.y = dy->y; a.gs = dy->scale; a.gt = dy->shift; a.gk1 = dy->k1; a.gk0 = dy->k0; a.gact = dy->act;
    a.ldy = ldy;
    a.M = m; a.K = k; a.N = n;
    return wgrad_run(ctx, a, dw);
}

}  // extern "C"
