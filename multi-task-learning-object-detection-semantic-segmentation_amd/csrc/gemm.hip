// Pointwise (1x1) convolution as GEMM on the fp32-input matrix cores (v_mfma_f32_32x32x2_f32: exact fp32
// products, fp32 accumulate -- the only MFMA dtype that keeps 1e-3 rel through ~60 layers without operand
// splitting).  Replaces Conv2D 1x1 / the pointwise half of SeparableConv2D (reference models.py:65,110;
// blocks.py:28,58,70,109) forward, backward-data and backward-weight.
//
//   fwd        y[m][n]  = sum_k act(scale_k*x[m][k]+shift_k) * w[k][n]         + per-channel (sum,sumsq) partials
//   bwd_data   dx[m][k] = sum_n dy[m][n] * w[k][n]   (+ residual, + accumulate)  dy formed on load (BN backward)
//   bwd_weight dw[k][n] = sum_m a[m][k] * dy[m][n]                               split over m, fixed-order reduce
//
// fwd/bwd_data share one kernel ("rowA": the streamed operand is row-major with the reduction axis contiguous).
// Tile: 128 rows x (32*WN) cols per 256-thread block, BK = 32.  The streamed operand is staged through LDS as
// [128][32+4] so that each lane fetches 4 consecutive k with one conflict-free ds_read_b128; since a GEMM may
// visit k in any order, MFMA #jj of a group takes k = 8*kk + jj from lanes 0-31 and k = 8*kk + 4 + jj from lanes
// 32-63 (for A and B alike).  The weight tile sits in LDS as [32][BN+1] and is read with conflict-free ds_read_b32.
// The next tile's global loads are issued before the current tile's MFMAs (register prefetch).
#include "gemm_internal.h"

namespace {

// (the kernels take these unit-local types, so that their symbols spell the argument type inside the unnamed namespace)
struct RowAArgs : ssdseg_rowa_args {};

// LD: how the streamed operand is addressed -- 0 plain row-major matrix, 1 dense 3x3 stride-1 gather, 2 stem gather
// NT > 0 (MODE 1, LD 0, WN 1, J <= 32, R <= 32*NT): fused backward of a pointwise conv with few input channels (the MBConv
// expand convs): the same pass over (g, y) that yields dx = dy * W^T also accumulates dW = a^T * dy, one 32x32 tile per
// 32-column chunk of dy, each wave over its own 32 rows -- so the 6x-wide gradient is read once instead of twice.
// BNE (MODE 1, LD 0, NT 0): float4 epilogue through LDS -- the 128 x BN tile leaves the accumulators in two 64-row halves,
// is re-read as rows of float4 (thread = fixed float4 column, several rows), added to residual / previous contents, stored
// with 16-byte lanes, and in the same pass reduced into the BatchNorm-backward sums of the layer that produced this conv's
// input (one extra read of that layer's raw output instead of a separate two-tensor reduction pass).
// EP: 0 = scalar epilogue straight from the accumulators, 1 = the float4 epilogue, 2 = float4 epilogue + BN backward sums
// occupancy targets (waves per SIMD; a block is 4 waves = one per SIMD): the widest tile used to land at 264-300 registers,
// i.e. ONE block per CU, where every barrier and every global->LDS hand-over idles the matrix pipe
// (measured: conv backward-data 77 -> 96 TFLOP/s at two blocks per CU, the HBM-bound early pointwise layers +20-50 %).
// OCC = 1 instantiations carry the target; OCC = 0 keeps the compiler's own allocation (accumulators in AGPRs, looser
// schedule), which is what the short-M late layers want: they are latency- not occupancy-bound (too few blocks to fill the
// chip twice anyway) and ran 10-25 % SLOWER with the tight allocation.  Dispatch: rows >= ROWA_OCC_ROWS.
constexpr int rowa_min_waves(int WN, int MODE, int NT) { return NT > 0 ? 2 : (WN >= 2 ? 2 : (MODE == 0 ? 4 : 3)); }
// (SSDSEG_OCC_ROWS: the parity tests flip it between calls to force either instantiation)
inline long long occ_rows() { return env_int("SSDSEG_OCC_ROWS", ROWA_OCC_ROWS); }
template <int WN, int MODE, int LD, int NT = 0, int EP = 0, int OCC = 0>
__global__ void __launch_bounds__(256, OCC ? rowa_min_waves(WN, MODE, NT) : 1) gemm_rowA_kernel(RowAArgs p) {
    constexpr bool CONV = LD == 1, STEM = LD == 2, FUSEW = NT > 0, F4 = EP >= 1, BNE = EP == 2;
    static_assert(!F4 || (LD == 0 && NT == 0), "float4 epilogue only for the plain pointwise GEMM");
    static_assert(!BNE || MODE == 1, "BN epilogue only for backward-data");
    static_assert(!FUSEW || (MODE == 1 && LD == 0 && WN == 1), "fused dW only for plain backward-data with one column tile");
    constexpr int BN = 32 * WN;
    constexpr int BS = BN + 1;
    extern __shared__ float smem[];
    float* As = smem;                 // [BM][AS]
    float* Bs = smem + BM * AS;       // [BK][BS]

    const int t = threadIdx.x;
    const int wave = t >> 6, lane = t & 63, li = lane & 31, hh = lane >> 5;
    const int j0 = blockIdx.x * BN;
    const int mtiles = (p.I + BM - 1) / BM;
    const int KT = (p.R + BK - 1) / BK;
    const bool affine = p.cs != nullptr;

    const int a_c4 = t & 7;
    const int a_r = t >> 3;
    float4 areg[4];
    float4 breg[WN];

    const float alo = act_lo(p.act), ahi = act_hi(p.act);
    const float* ya = affine ? p.a1 : p.a0;                       // identity gradient view: y aliases g, act NONE
    const int gact = affine ? p.act : SSDSEG_ACT_NONE;
    int m0 = 0;
    int rn[4], rh[4], rw[4];   // CONV: (image, row, col) of this thread's 4 staged rows, fixed for a row tile
    auto load_tiles = [&](int kt) {
        const int r = kt * BK + a_c4 * 4;
        const bool rin = r < p.R;
        int ch = r, dh = 0, dw = 0;   // channel inside the tap, spatial offset of the tap
        if (CONV) {
            const int tap = r / p.convC;
            ch = r - tap * p.convC;
            const int kh = tap / 3;
            dh = (kh - 1) * p.convSign;
            dw = (tap - kh * 3 - 1) * p.convSign;
        }
        float4 cs = f4(1.f), ct = f4(0.f), ck1 = f4(0.f), ck0 = f4(0.f);   // identity view unless per-channel coefficients exist
        if (affine && rin) {
            cs = ld4(p.cs + ch);
            ct = ld4(p.ct + ch);
            if (MODE == 1) { ck1 = ld4(p.ck1 + ch); ck0 = ld4(p.ck0 + ch); }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + a_r + 32 * i;
            float4 v = f4(0.f);
            bool ok = rin && m < p.I;
            long long off = (long long)m * p.lda + r;
            if (CONV) {
                const int sh = rh[i] + dh, sw = rw[i] + dw;
                ok = ok && sh >= 0 && sh < p.convH && sw >= 0 && sw < p.convW;
                off = (((long long)rn[i] * p.convH + sh) * p.convW + sw) * p.lda + ch;
            }
            if (STEM) {
                // four scalar gathers: r .. r+3 are (kh, kw, ci) triples of a 3-channel pixel row, not 16-byte aligned
                float e[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int rq = r + q, tap = rq / 3, ci = rq - tap * 3, kh = tap / 3, kw = tap - kh * 3;
                    const int hi = 2 * rh[i] + kh - p.stemPt, wi = 2 * rw[i] + kw - p.stemPl;
                    const bool okq = rq < p.R && m < p.I && hi >= 0 && hi < p.stemH && wi >= 0 && wi < p.stemW;
                    const long long o = okq ? (((long long)rn[i] * p.stemH + hi) * p.stemW + wi) * 3 + ci : 0;
                    const float x = p.a0[o];
                    e[q] = okq ? fmaf(x, p.stemScale, p.stemOffset) : 0.f;
                }
                areg[i] = make_float4(e[0], e[1], e[2], e[3]);
                continue;
            }
            // unconditional loads from a clamped address + select: the 4 row loads (and their twins for y) issue back to back
            if (!ok) off = 0;
            if (MODE == 0) v = view_affine4(ld4(p.a0 + off), cs, ct, alo, ahi);
            else v = gview_apply4(ld4(p.a0 + off), ld4(ya + off), cs, ct, ck1, ck0, gact);
            areg[i] = ok ? v : f4(0.f);
        }
#pragma unroll
        for (int q = 0; q < WN; ++q) {
            const int idx = t + 256 * q;
            float4 v = f4(0.f);
            if (MODE == 0) {
                const int rr = idx / (8 * WN), j4 = idx % (8 * WN);
                const int gr = kt * BK + rr, gj = j0 + j4 * 4;
                const bool bok = gr < p.R && gj < p.J;
                v = ld4(p.b + (bok ? (long long)gr * p.ldb + gj : 0));
                if (!bok) v = f4(0.f);
            } else {
                const int jj = idx >> 3, r4 = idx & 7;
                const int gr = kt * BK + r4 * 4, gj = j0 + jj;
                // CONV: w[tap][j][c] with r = tap*convC + c  ->  j*convC + r + tap*convC*(J-1)
                const long long tapoff = CONV ? (long long)(gr / p.convC) * p.convC * (p.J - 1) : 0;
                const bool bok = gr < p.R && gj < p.J;
                v = ld4(p.b + (bok ? (long long)gj * p.ldb + gr + tapoff : 0));
                if (!bok) v = f4(0.f);
            }
            breg[q] = v;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) st4(As + (a_r + 32 * i) * AS + a_c4 * 4, areg[i]);
#pragma unroll
        for (int q = 0; q < WN; ++q) {
            const int idx = t + 256 * q;
            if (MODE == 0) {
                const int rr = idx / (8 * WN), j4 = idx % (8 * WN);
                float* d = Bs + rr * BS + j4 * 4;
                d[0] = breg[q].x; d[1] = breg[q].y; d[2] = breg[q].z; d[3] = breg[q].w;
            } else {
                const int jj = idx >> 3, r4 = idx & 7;
                float* d = Bs + (r4 * 4) * BS + jj;
                d[0] = breg[q].x; d[BS] = breg[q].y; d[2 * BS] = breg[q].z; d[3 * BS] = breg[q].w;
            }
        }
    };

    float ssum[WN], ssq[WN];   // BN statistics of this block's rows, carried across its row tiles
#pragma unroll
    for (int nt = 0; nt < WN; ++nt) ssum[nt] = ssq[nt] = 0.f;
    f32x16 wacc[FUSEW ? NT : 1];   // FUSEW: this wave's partial of dW[j][32*kt + ..] over its rows, carried across row tiles
#pragma unroll
    for (int q = 0; q < (FUSEW ? NT : 1); ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) wacc[q][e] = 0.f;
    float xop[FUSEW ? 16 : 1];     // FUSEW: A operand a[m0 + 32*wave + 2s + hh][j = li] of the dW products, per row tile
    // BNE: this thread's float4 column of the epilogue and its BatchNorm constants / running sums
    float4 ebs = f4(0.f), ebt = f4(0.f), ebm = f4(0.f), ebi = f4(0.f), esb = f4(0.f), esg = f4(0.f);
    const float bnlo = act_lo(p.bn_act), bnhi = act_hi(p.bn_act);
    if (BNE) {
        const int ec4 = t % (BN / 4), ej = j0 + ec4 * 4;
        if (ej < p.J) { ebs = ld4(p.bn_s + ej); ebt = ld4(p.bn_t + ej); ebm = ld4(p.bn_mean + ej); ebi = ld4(p.bn_istd + ej); }
    }

    // a block walks row tiles blockIdx.y, blockIdx.y + gridDim.y, ... so the number of BN partial rows stays small
    for (int mt = blockIdx.y; mt < mtiles; mt += gridDim.y) {
    m0 = mt * BM;
    if (CONV || STEM) {
        const int hw = p.convH * p.convW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + a_r + 32 * i;
            rn[i] = m / hw;
            const int rem = m - rn[i] * hw;
            rh[i] = rem / p.convW;
            rw[i] = rem - rh[i] * p.convW;
        }
    }
    f32x16 acc[WN], accb;
#pragma unroll
    for (int nt = 0; nt < WN; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) accb[e] = 0.f;

    if (FUSEW) {
        const float xlo = act_lo(p.xwact), xhi = act_hi(p.xwact);
        const bool jok = li < p.J;
        const float xs = (p.xws != nullptr && jok) ? p.xws[li] : 1.f, xt = (p.xws != nullptr && jok) ? p.xwt[li] : 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int m = m0 + wave * 32 + 2 * s + hh;
            const bool ok = jok && m < p.I;
            const float v = p.xw[ok ? (long long)m * p.ldxw + li : 0];
            xop[s] = ok ? fminf(fmaxf(fmaf(xs, v, xt), xlo), xhi) : 0.f;
        }
    }
    const int kt0 = 0, kt1 = KT;
    load_tiles(kt0);
    // one 32-deep reduction step; `wtile` = which dW accumulator this step feeds (a compile-time constant in the fused loop)
    auto kstep = [&](int kt, f32x16& wtile) {
        __syncthreads();
        store_tiles();
        __syncthreads();
        if (kt + 1 < kt1) load_tiles(kt + 1);
        if (FUSEW) {
            // dW tile kt: rows of the reduction = this wave's 32 tile rows, B operand dy[row][32*kt + li] straight from As
            const float* dcol = As + (wave * 32 + hh) * AS + li;
#pragma unroll
            for (int s = 0; s < 16; ++s) wtile = mfma32(xop[s], dcol[(2 * s) * AS], wtile);
        }
        const float* arow = As + (wave * 32 + li) * AS + 4 * hh;
        const float* bcol = Bs + (4 * hh) * BS + li;
        // Operand fragments are read from LDS one 8-deep group AHEAD of the MFMAs that use them (two register sets).  Left
        // to itself the compiler put each ds_read right in front of its MFMA with an s_waitcnt lgkmcnt(0), so the matrix
        // pipe idled for an LDS round trip every 1-2 instructions (38-59 TFLOP/s on the compute-bound layers).
        float4 afr[2];
        float bfr[2][4][WN];
        auto fetch = [&](int kk, int buf) {
            afr[buf] = ld4(arow + kk * 8);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int nt = 0; nt < WN; ++nt) bfr[buf][jj][nt] = bcol[(kk * 8 + jj) * BS + nt * 32];
        };
        fetch(0, 0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk + 1 < 4) fetch(kk + 1, (kk + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);   // keep the reads of group kk+1 in front of the MFMAs of group kk
            const float av[4] = {afr[kk & 1].x, afr[kk & 1].y, afr[kk & 1].z, afr[kk & 1].w};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                for (int nt = 0; nt < WN; ++nt) {
                    // one column tile: alternate between two accumulators so consecutive MFMAs are independent
                    if (WN == 1 && (jj & 1)) accb = mfma32(av[jj], bfr[kk & 1][jj][nt], accb);
                    else acc[nt] = mfma32(av[jj], bfr[kk & 1][jj][nt], acc[nt]);
                }
            }
        }
    };
    if (FUSEW) {
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            if (kt < KT) kstep(kt, wacc[kt]);
    } else {
        for (int kt = kt0; kt < kt1; ++kt) kstep(kt, wacc[0]);
    }
    if (WN == 1) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[0][e] += accb[e];
    }

    if (F4) {
        constexpr int CS = BN + 4;        // LDS row stride of the transposed tile (float4-aligned)
        constexpr int CV = BN / 4;        // float4 columns
        constexpr int RPP = 256 / CV;     // rows per pass of the 256 threads
        float* Cs = smem;                 // [64][CS], over As/Bs (all waves are past their last operand read after the barrier)
        const int er = t / CV, ec4 = t - er * CV;
        const int ej = j0 + ec4 * 4;
        const bool eact = er < RPP && ej < p.J;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __syncthreads();
            if ((wave >> 1) == h) {
#pragma unroll
                for (int nt = 0; nt < WN; ++nt)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        Cs[((wave & 1) * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh) * CS + nt * 32 + li] = acc[nt][e];
            }
            __syncthreads();
            if (eact) {
                // Rows er, er + RPP, ... of this half, FOUR at a time: the global loads of a group (the raw input of the fused
                // BatchNorm sums, residual, previous dx) are issued together and the group is then consumed in row order -- the
                // summation order per thread is unchanged.  One row per trip left a single 16-byte load in flight per thread
                // (8 KB per CU): the project-conv backward GEMMs of blocks 0-3 ran at 2.2-3.3 TB/s of real traffic.
                // Only where the registers are there (<= 3 column tiles, the register-limited big-M instantiations): at 4-5 column
                // tiles the extra float4s spill (block-2 project conv +11 %), and the short-M instantiations would lose a wave per SIMD.
                constexpr int ITER = (64 + RPP - 1) / RPP;
                constexpr int EU = (OCC && WN <= 3) ? 4 : 1;
                if constexpr (EU == 1) {
                // one row per trip, the raw input of the fused BatchNorm sums fetched one row AHEAD (two loads in flight per thread
                // for four more registers)
                float4 ynext = f4(0.f);
                if (BNE && m0 + h * 64 + er < p.I) ynext = ld4(p.bn_y + (long long)(m0 + h * 64 + er) * p.ldby + ej);
                for (int row = er; row < 64; row += RPP) {
                    const int m = m0 + h * 64 + row;
                    if (m >= p.I) break;
                    const float4 yv = ynext;
                    if (BNE && row + RPP < 64 && m + RPP < p.I) ynext = ld4(p.bn_y + (long long)(m + RPP) * p.ldby + ej);
                    float4 v = ld4(Cs + row * CS + ec4 * 4);
                    if (MODE == 1 && p.residual) {
                        const float4 r4 = ld4(p.residual + (long long)m * p.ldr + ej);
                        v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
                    }
                    float* o = p.out + (long long)m * p.ldo + ej;
                    if (MODE == 1 && p.accumulate) {
                        const float4 o4 = ld4(o);
                        v.x += o4.x; v.y += o4.y; v.z += o4.z; v.w += o4.w;
                    }
                    st4(o, v);
                    if (!BNE) continue;
                    float4 mg;
                    mg.x = (fmaf(ebs.x, yv.x, ebt.x) > bnlo && fmaf(ebs.x, yv.x, ebt.x) < bnhi) ? v.x : 0.f;
                    mg.y = (fmaf(ebs.y, yv.y, ebt.y) > bnlo && fmaf(ebs.y, yv.y, ebt.y) < bnhi) ? v.y : 0.f;
                    mg.z = (fmaf(ebs.z, yv.z, ebt.z) > bnlo && fmaf(ebs.z, yv.z, ebt.z) < bnhi) ? v.z : 0.f;
                    mg.w = (fmaf(ebs.w, yv.w, ebt.w) > bnlo && fmaf(ebs.w, yv.w, ebt.w) < bnhi) ? v.w : 0.f;
                    esb.x += mg.x; esb.y += mg.y; esb.z += mg.z; esb.w += mg.w;
                    esg.x = fmaf(mg.x, (yv.x - ebm.x) * ebi.x, esg.x); esg.y = fmaf(mg.y, (yv.y - ebm.y) * ebi.y, esg.y);
                    esg.z = fmaf(mg.z, (yv.z - ebm.z) * ebi.z, esg.z); esg.w = fmaf(mg.w, (yv.w - ebm.w) * ebi.w, esg.w);
                }
                } else {
#pragma unroll
                for (int it0 = 0; it0 < ITER; it0 += EU) {
                    float4 cv[EU], yv4[EU], rv4[EU], ov4[EU];
                    bool rok[EU];
#pragma unroll
                    for (int u = 0; u < EU; ++u) {
                        const int row = er + (it0 + u) * RPP;
                        const int m = m0 + h * 64 + row;
                        rok[u] = (it0 + u) < ITER && row < 64 && m < p.I;
                        const long long mm = rok[u] ? m : 0;               // clamped address, value unused
                        if (BNE) yv4[u] = ld4(p.bn_y + mm * p.ldby + ej);
                        if (MODE == 1 && p.residual) rv4[u] = ld4(p.residual + mm * p.ldr + ej);
                        if (MODE == 1 && p.accumulate) ov4[u] = ld4(p.out + mm * p.ldo + ej);
                        cv[u] = ld4(Cs + (rok[u] ? row : 0) * CS + ec4 * 4);
                    }
#pragma unroll
                    for (int u = 0; u < EU; ++u) {
                        if (!rok[u]) continue;
                        const int m = m0 + h * 64 + er + (it0 + u) * RPP;
                        float4 v = cv[u];
                        if (MODE == 1 && p.residual) { v.x += rv4[u].x; v.y += rv4[u].y; v.z += rv4[u].z; v.w += rv4[u].w; }
                        if (MODE == 1 && p.accumulate) { v.x += ov4[u].x; v.y += ov4[u].y; v.z += ov4[u].z; v.w += ov4[u].w; }
                        st4(p.out + (long long)m * p.ldo + ej, v);
                        if (!BNE) continue;
                        const float4 yv = yv4[u];
                        float4 mg;
                        mg.x = (fmaf(ebs.x, yv.x, ebt.x) > bnlo && fmaf(ebs.x, yv.x, ebt.x) < bnhi) ? v.x : 0.f;
                        mg.y = (fmaf(ebs.y, yv.y, ebt.y) > bnlo && fmaf(ebs.y, yv.y, ebt.y) < bnhi) ? v.y : 0.f;
                        mg.z = (fmaf(ebs.z, yv.z, ebt.z) > bnlo && fmaf(ebs.z, yv.z, ebt.z) < bnhi) ? v.z : 0.f;
                        mg.w = (fmaf(ebs.w, yv.w, ebt.w) > bnlo && fmaf(ebs.w, yv.w, ebt.w) < bnhi) ? v.w : 0.f;
                        esb.x += mg.x; esb.y += mg.y; esb.z += mg.z; esb.w += mg.w;
                        esg.x = fmaf(mg.x, (yv.x - ebm.x) * ebi.x, esg.x); esg.y = fmaf(mg.y, (yv.y - ebm.y) * ebi.y, esg.y);
                        esg.z = fmaf(mg.z, (yv.z - ebm.z) * ebi.z, esg.z); esg.w = fmaf(mg.w, (yv.w - ebm.w) * ebi.w, esg.w);
                    }
                }
                }
            }
        }
        __syncthreads();   // the tile is consumed: the next row tile may overwrite As/Bs
    } else {
    // ---------------- epilogue: C/D layout col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
#pragma unroll
    for (int nt = 0; nt < WN; ++nt) {
        const int j = j0 + nt * 32 + li;
        if (j < p.J) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                if (m < p.I) {
                    float v = acc[nt][e];
                    if (STEM && p.bias) v += p.bias[j];
                    if (MODE == 1) {
                        if (p.residual) v += p.residual[(long long)m * p.ldr + j];
                        if (p.accumulate) v += p.out[(long long)m * p.ldo + j];
                    }
                    p.out[(long long)m * p.ldo + j] = v;
                }
            }
        }
    }
    }   // !F4
    if (MODE == 0 && p.stats != nullptr) {
        // per-channel (sum, sumsq) of this 128-row tile; padded rows are exactly zero
#pragma unroll
        for (int nt = 0; nt < WN; ++nt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) { ssum[nt] += acc[nt][e]; ssq[nt] = fmaf(acc[nt][e], acc[nt][e], ssq[nt]); }
        }
    }
    }  // row-tile loop

    if (FUSEW) {
        // this block's dW partial slab [J][R]: sum the four waves' row-quarters tile by tile through LDS (fixed order)
        float* red = smem;   // [3 waves][16][64]
        float* slab = p.wpart + (long long)blockIdx.y * p.J * p.R;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            __syncthreads();
            if (wave > 0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) red[((wave - 1) * 16 + e) * 64 + lane] = wacc[kt][e];
            }
            __syncthreads();
            if (wave == 0) {
                const int n = kt * 32 + li;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = ((wacc[kt][e] + red[(0 * 16 + e) * 64 + lane]) + red[(1 * 16 + e) * 64 + lane]) + red[(2 * 16 + e) * 64 + lane];
                    const int k = (e & 3) + 8 * (e >> 2) + 4 * hh;
                    if (k < p.J && n < p.R) slab[(long long)k * p.R + n] = v;
                }
            }
        }
    }

    if (BNE) {
        // fold the threads that share a float4 column (fixed order) -> this block's partial row
        constexpr int CV = BN / 4, RPP = 256 / CV;
        float4* red4 = reinterpret_cast<float4*>(smem);   // [2][256]
        __syncthreads();
        red4[t] = esb;
        red4[256 + t] = esg;
        __syncthreads();
        if (t < CV && j0 + t * 4 < p.J) {
            float4 a = f4(0.f), b = f4(0.f);
            for (int k = 0; k < RPP; ++k) {
                const float4 x = red4[k * CV + t], y = red4[256 + k * CV + t];
                a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
                b.x += y.x; b.y += y.y; b.z += y.z; b.w += y.w;
            }
            st4(p.bnpart + ((long long)blockIdx.y * 2 + 0) * p.J + j0 + t * 4, a);
            st4(p.bnpart + ((long long)blockIdx.y * 2 + 1) * p.J + j0 + t * 4, b);
        }
    }
    if (MODE == 0 && p.stats != nullptr) {
        __syncthreads();
        float* red = smem;  // [4 waves][2][BN]
#pragma unroll
        for (int nt = 0; nt < WN; ++nt) {
            float s = ssum[nt], q = ssq[nt];
            s += __shfl_xor(s, 32, 64);
            q += __shfl_xor(q, 32, 64);
            if (hh == 0) {
                red[(wave * 2 + 0) * BN + nt * 32 + li] = s;
                red[(wave * 2 + 1) * BN + nt * 32 + li] = q;
            }
        }
        __syncthreads();
        for (int idx = t; idx < 2 * BN; idx += 256) {
            const int which = idx / BN, jl = idx % BN;
            const int j = j0 + jl;
            if (j < p.J) {
                float v = red[(0 * 2 + which) * BN + jl] + red[(1 * 2 + which) * BN + jl] + red[(2 * 2 + which) * BN + jl] +
                          red[(3 * 2 + which) * BN + jl];
                p.stats[((long long)blockIdx.y * 2 + which) * p.J + j] = v;
            }
        }
    }
}


int rowA_wn(int rows, int cols);
// Backward-data GEMMs with a tiny reduction (<= 48 channels: the project convs of blocks 1-3, the decoder's backbone / logits convs)
// are all epilogue: 128 x 144 outputs per 128 x 24 inputs.  At 4-5 column tiles the float4 epilogue walks 11 rows per thread with
// one load in flight; at <= 3 it takes four rows at a time (gemm_rowA_kernel, EU) -- two 96- / 72-column tiles beat one of 144 / 160
// although the narrow operand is read twice (block-2 project conv 379 -> 277 us).  Only for the register-limited big-M instantiations.
int rowA_wn_bwd(int rows, int cols, int red) {
    const int wn = rowA_wn(rows, cols);
    const int cap = (int)env_int("SSDSEG_ROWA_BWD_WN", 3);         // (A/B runs) "0": no cap
    return (cap >= 1 && rows >= occ_rows() && red <= 48 && wn > cap) ? cap : wn;
}
int rowA_wn(int rows, int cols) {
    const int wn = pick_wn(cols, cdiv(rows, BM));
    const int cap = (int)env_int("SSDSEG_ROWA_WN_MAX", 0);        // (A/B runs) widest column tile, in 32-column units
    return (cap >= 1 && wn > cap) ? cap : wn;
}

#include "gemm_wres.h"
#include "pw_tile.h"

// ---- tile GEMM of the pointwise convs (pw_tile.h): shape -> (waves, column tile), launch
// SSDSEG_PW_TILE: "0" never, "1" every shape the kernel takes, unset: where it measured faster
int pw_tile_mode() {
    return getenv("SSDSEG_PW_TILE") == nullptr ? 2 : (env_is("SSDSEG_PW_TILE", '0') ? 0 : 1);
}

template <int WAVES, int WN, int MODE, int WNW = 1>
int pwt_launch_inst(ssdseg_ctx* ctx, const PwTArgs& a, dim3 grid, double cost_bytes, double cost_flops) {
    const size_t lds = pwt_lds_floats(32 * WAVES / WNW, 32 * WN * WNW, a.cred) * sizeof(float);
    static size_t configured = 0;
    if (lds > configured) {
        SSDSEG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pw_tile_kernel<WAVES, WN, MODE, WNW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        configured = lds;
    }
    char kbuf[64];
    if (WNW == 1) snprintf(kbuf, sizeof(kbuf), "pw_tile_kernel<%d, %d, %d>", WAVES, WN, MODE);
    else snprintf(kbuf, sizeof(kbuf), "pw_tile_kernel<%d, %d, %d, %d>", WAVES, WN, MODE, WNW);
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, (pw_tile_kernel<WAVES, WN, MODE, WNW>), grid, dim3(64 * WAVES), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// default dispatch rule, read off the per-layer A/B table (profiles/r02_pw_tile_vs_rowA_per_layer.txt)
// (round 2, one MI355X, batch 32).  Forward: every layer with >= 256 output channels (the expand convs of the 30x40 / 15x20
// stages, the ASPP branches and output conv, the decoder sepconv: 0.83-0.95 of the rowA time; project convs with <= 160 outputs
// lose 1.0-1.9x: too few, too narrow tiles) and the 36-column tap-expanded GEMM of the 256 -> 4 logits conv (614,400 rows).
// Input gradient: plain epilogues (no fused BatchNorm sums, no accumulation into an existing gradient: the tile kernel's scalar
// epilogue loses there) with a reduction of <= 384 channels and a wide side (>= 256) somewhere: decoder sepconv 0.76, encoder
// output conv 0.80, expand convs of blocks 7-10 0.84-0.93, ASPP atrous branches 0.93-0.98; long reductions onto few columns
// (expand convs of blocks 11-16: one column tile, 75-300 blocks) lose 1.1-1.4x.
// Round 2, second table (profiles/r02_pw_tile_short_m_per_layer.txt): with 64- / 32-column tiles the tile kernel also wins every
// FORWARD below 65,536 rows (project convs of the 30x40 / 15x20 stages 0.8, the SSD head and extra-feature-map convs 0.45-0.8) and the
// plain input gradients of <= 16k rows (expand convs of blocks 14-16: 0.75-0.85, extra feature maps 0.45).
bool pw_tile_default(int mode, long long rows, int cred, int nout, bool fused_bn, bool accumulate) {
    const bool pinned = env_is("SSDSEG_PWT_SMALL", '0');
    if (mode == 0) return nout >= 256 || (rows >= 500000 && cred >= 256) || (rows < 65536 && !pinned);
    if (!fused_bn && !accumulate && rows <= 16384 && !pinned) return true;
    return !fused_bn && !accumulate && cred <= 384 && (nout >= 256 || cred >= 256);
}

// can the tile kernel take this GEMM?  (reduction a multiple of 8 and at least two steps deep; 32-bit buffer offsets)
bool pw_tile_takes(long long rows, int lda, int cred, int nout) {
    return cred % 8 == 0 && cred >= 64 && nout % 4 == 0 && rows * (long long)lda * 4 < (1LL << 31) && (long long)nout * cred * 4 < (1LL << 31);
}

// THE tile-GEMM question, asked by the forward (launch_rowA), by ssdseg_pwconv_wt_floats -- which tells the engine at lowering
// whether to keep a transposed weight copy for it -- and by the fused BatchNorm input gradient: does the tile kernel run this layer?
bool pw_tile_wanted(int mode, long long rows, int lda, int cred, int nout, bool fused_bn, bool accumulate_or_residual) {
    const int sw = pw_tile_mode();
    return sw != 0 && pw_tile_takes(rows, lda, cred, nout) && (sw == 1 || pw_tile_default(mode, rows, cred, nout, fused_bn, accumulate_or_residual));
}

// Short-M layers (the 30x40 / 15x20 stages and the extra feature maps: 38,400 / 9,600 / 2,560 ... rows at batch 32): 128-row tiles
// give 300 / 75 / 20 row tiles for 256 CUs, so the column tile is what makes the blocks.  Measured per layer
// (profiles/r02_pw_tile_short_m_per_layer.txt; blocks of one or two waves lost everywhere: every block stages its own weight
// tile, and LDS then holds three waves per CU): 64-column tiles, 32 where 64 would pad more than a quarter, 32 for <= 16k rows.
// SSDSEG_PWT_SMALL=<ncols> overrides the width for A/B runs, "0" restores one tile of <= 160 columns.
constexpr int PWT_SHORT_ROWS = 65536;
int pwt_short_ncols(int mode, long long rows, int cred, int nout) {
    if (getenv("SSDSEG_PWT_SMALL") != nullptr) {
        const int nc = (int)env_int("SSDSEG_PWT_SMALL", 0);
        return nc >= 32 ? nc : 0;
    }
    const int t64 = cdiv(nout, 64);
    const bool pad64 = cdiv((cdiv(nout, t64) + 3) / 4 * 4, 32) * 32 * t64 * 4 > nout * 5;
    if (mode == 0) {
        if (rows <= 16384) return nout >= 512 ? 0 : 32;
        if (cred <= 64) return 128;
        return (nout <= 64 || pad64) ? 32 : 64;
    }
    if (rows <= 16384) return 32;
    return nout <= 64 ? 64 : (pad64 ? 32 : 64);
}

// Blocks along y of a tile-GEMM launch that is free to choose == rows of the BatchNorm-backward partial table its caller sizes:
// one per `block_rows` rows, at most 1024 blocks per launch over the gx column tiles (SSDSEG_PWT_PARTS >= 64, A/B runs: that many).
// (ssdseg_pwconv_bwd_data_bn sizes by 256-row blocks from 65,536 rows and one column tile; a block walks row tiles
// blockIdx.y, blockIdx.y + gridDim.y, ..., so any count is valid for the 128-row blocks of the 4 x 2 wave grid as well)
int pwt_part_rows(long long rows, int block_rows, int gx) {
    const int mtiles = cdiv(rows, block_rows);
    const int parts = (int)env_int("SSDSEG_PWT_PARTS", 0);
    const int cap = (parts >= 64 ? parts : 1024 * gx) / gx;
    const int gy = mtiles < cap ? mtiles : cap;
    return gy < 1 ? 1 : gy;
}

// nparts_y: number of blocks along y == number of partial rows the caller sized its statistics table for (0: free choice)
template <int MODE>
int pw_tile_launch(ssdseg_ctx* ctx, PwTArgs a, int nparts_y, double view_bytes) {
    int ntiles = a.nout <= 160 ? 1 : cdiv(a.nout, 256);
    if (a.M < PWT_SHORT_ROWS) {
        const int nc = pwt_short_ncols(MODE, a.M, a.cred, a.nout);
        if (nc > 0) ntiles = cdiv(a.nout, nc);
    }
    a.ncols = (cdiv(a.nout, ntiles) + 3) / 4 * 4;
    int wn = cdiv(a.ncols, 32);
    // >= 256 row tiles of 256 rows: eight-wave blocks, one per CU  (SSDSEG_PW_TILE_BIG_ROWS, A/B runs: rows from which they are used)
    const bool big = a.M >= env_int("SSDSEG_PW_TILE_BIG_ROWS", 65536);
    // column tiles of <= 160: four-wave blocks (two blocks per CU), and the input-gradient kernel whatever its size (its gradient
    // view staging and epilogue need ~60 registers more: 6- and 8-tile instantiations spill)
    if ((!big || MODE == 1) && wn > 5) {
        const int nt2 = cdiv(a.nout, 160);
        a.ncols = (cdiv(a.nout, nt2) + 3) / 4 * 4;
        wn = cdiv(a.ncols, 32);
    }
    // input gradient with 161 .. 256 output columns at >= 65,536 rows (the decoder sepconv): a 4 x 2 wave grid over a 128-row block
    // that spans ALL columns -- the two-tensor operand is streamed once, not once per 128-column tile (SSDSEG_PWT_GRID=0: off)
    const bool grid42 = MODE == 1 && big && a.nout > 160 && a.nout <= 256 && !env_is("SSDSEG_PWT_GRID", '0');
    if (grid42) { a.ncols = (a.nout + 3) / 4 * 4; wn = cdiv(a.ncols, 64); }
    const int gx = cdiv(a.nout, a.ncols);
    const int gy = nparts_y > 0 ? nparts_y : pwt_part_rows(a.M, (big && !grid42) ? 256 : 128, gx);
    a.a_bytes = (unsigned)((((long long)a.M - 1) * a.lda + a.cred) * 4);
    a.wt_bytes = (unsigned)((long long)a.nout * a.cred * 4);
    const dim3 grid(gx, gy, 1);
    const double cost_bytes = 4.0 * ((double)a.M * a.cred + (double)a.M * a.nout + (double)a.cred * a.nout);
    const double cost_flops = 2.0 * a.M * a.cred * a.nout;
    ctx->timing_view_bytes = view_bytes;
#define PWT_CASE(W, N) return pwt_launch_inst<W, N, MODE>(ctx, a, grid, cost_bytes, cost_flops)
    if constexpr (MODE == 1) {
        if (grid42) {
            if (wn <= 3) return pwt_launch_inst<8, 3, MODE, 2>(ctx, a, grid, cost_bytes, cost_flops);
            return pwt_launch_inst<8, 4, MODE, 2>(ctx, a, grid, cost_bytes, cost_flops);
        }
    }
    if (big) {
        if (wn <= 2) PWT_CASE(8, 2);
        if (wn <= 4) PWT_CASE(8, 4);
        if (wn == 5) PWT_CASE(8, 5);
        if constexpr (MODE == 0) {
            if (wn == 6) PWT_CASE(8, 6);
            PWT_CASE(8, 8);
        }
    }
    if (wn <= 1) PWT_CASE(4, 1);
    if (wn <= 2) PWT_CASE(4, 2);
    if (wn <= 3) PWT_CASE(4, 3);
    if (wn <= 4) PWT_CASE(4, 4);
    PWT_CASE(4, 5);
#undef PWT_CASE
}

// 1: the resident kernels where they measured faster (default); 0: SSDSEG_NO_WRES=1, general kernels everywhere (A/B
// measurements); 2: SSDSEG_WRES_FORCE=1, resident kernels for every shape that fits (the parity tests run that way)
int wres_mode() {
    // (read on every call, not cached: the parity tests flip these between calls)
    return env_is("SSDSEG_NO_WRES", '1') ? 0 : (env_is("SSDSEG_WRES_FORCE", '1') ? 2 : 1);
}
bool wres_enabled() { return wres_mode() != 0; }

// row-tile slots per column tile: enough blocks to fill the chip (~8 per CU), few enough that the BN partial
// table stays short
int rowA_grid_y_wn(int rows, int cols, int wn);
int rowA_grid_y(int rows, int cols) { return rowA_grid_y_wn(rows, cols, rowA_wn(rows, cols)); }
int rowA_grid_y_wn(int rows, int cols, int wn) {
    const int ntiles = cdiv(cols, 32 * wn), mtiles = cdiv(rows, BM);
    const int parts = (int)env_int("SSDSEG_ROWA_PARTS", 0);      // (A/B runs) cap of row-tile slots x column tiles
    // two blocks per CU for the 2-5 tile instantiations; the one-tile ones are compiled for four (three) blocks per CU
    // (rowa_min_waves) and want them: the stem conv ran 225 us on 2048 blocks, 316 us on 512
    const int cap = parts >= 64 ? parts : (wn == 1 ? 1024 : 512);
    // few tiles (the short-M stages): one row tile per block -- 75 row tiles dealt to 51 blocks is 2 rounds instead of 1
    if ((long long)mtiles * ntiles <= 2 * cap) return mtiles;
    int gy = cap / ntiles;
    if (gy < 1) gy = 1;
    if (mtiles <= gy) return mtiles;
    const int per = cdiv(mtiles, gy);       // row tiles per block, then as few blocks as carry them: an even deal
    return cdiv(mtiles, per);
}

// Algorithmic bytes and flops of one rowA / resident launch: read the streamed operand and the weights once, write
// the output once; the fused dx + dW pass (NT > 0) also reads X and writes dW.  The dense 3x3 conv (LD == 1) streams its input
// ONCE per 8(d) -- X + Y + W, not the nine-fold im2col operand the implicit GEMM walks (a.R = 9 * channels).  `view_bytes`: the
// second tensor of a BatchNorm-backward gradient view (raw y next to g) and, with the fused BatchNorm-backward epilogue (EP == 2),
// the raw input tensor it reads in place of that BN's own reduction pass.
struct GemmCost { double bytes, flops, view_bytes; };
template <int MODE, int LD, int NT, int EP>
GemmCost rowa_cost(const RowAArgs& a) {
    const double red_once = LD == 1 ? (double)a.convC : (double)a.R;
    GemmCost c;
    c.bytes = 4.0 * ((double)a.I * red_once + (NT > 0 ? 2.0 : 1.0) * ((double)a.I * a.J + (double)a.R * a.J));
    c.flops = (NT > 0 ? 4.0 : 2.0) * a.I * a.R * a.J;
    c.view_bytes = ((MODE == 1 && a.cs != nullptr) ? 4.0 * a.I * red_once : 0.0) + (EP == 2 ? 4.0 * a.I * a.J : 0.0);
    return c;
}

// THE launch of gemm_rowA_kernel.  LDS: the streamed tile + the weight tile, the statistics reduction scratch, and the
// 64 x (32 WN + 4) transpose slab of the float4 epilogues, whichever is largest.
template <int WN, int MODE, int LD, int NT, int EP, int OCC>
int rowa_launch_inst(ssdseg_ctx* ctx, const RowAArgs& a, dim3 grid) {
    constexpr size_t tile = (size_t)(BM * AS + BK * (32 * WN + 1)) * sizeof(float);
    constexpr size_t red = (size_t)(4 * 2 * 32 * WN) * sizeof(float);
    constexpr size_t slab = EP >= 1 ? (size_t)64 * (32 * WN + 4) * sizeof(float) : 0;
    constexpr size_t lds = tile > red ? (tile > slab ? tile : slab) : (red > slab ? red : slab);
    const GemmCost c = rowa_cost<MODE, LD, NT, EP>(a);
    ctx->timing_view_bytes = c.view_bytes;
    const char* kname = "";
    if (ctx->timing) {
        char kbuf[64];
        snprintf(kbuf, sizeof(kbuf), "gemm_rowA_kernel<%d, %d, %d, %d, %d, %d>", WN, MODE, LD, NT, EP, OCC);   // = the symbol rocprofv3 shows
        kname = ssdseg_intern(kbuf);
    }
    SSDSEG_LAUNCH_NAMED(ctx, kname, c.bytes, c.flops, (gemm_rowA_kernel<WN, MODE, LD, NT, EP, OCC>), grid, dim3(256), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
// column-tile width wn in [LO, 5], the occupancy-limited instantiation from occ_rows() rows
template <int MODE, int LD, int EP, int LO>
int rowa_launch(ssdseg_ctx* ctx, const RowAArgs& a, int wn, dim3 grid) {
    return for_width_occ<LO, 5>(wn, a.I >= occ_rows(), [&](auto W, auto OCC) {
        return rowa_launch_inst<decltype(W)::value, MODE, LD, 0, EP, decltype(OCC)::value>(ctx, a, grid);
    });
}

// THE launch of gemm_wres_kernel: whole weight slab resident in LDS, barrier-free per-wave streaming (gemm_wres.h)
template <int WN, int MODE, int NT>
int wres_launch_inst(ssdseg_ctx* ctx, const RowAArgs& a, dim3 grid) {
    const GemmCost c = rowa_cost<MODE, 0, NT, 0>(a);
    ctx->timing_view_bytes = c.view_bytes;
    const char* kname = "";
    if (ctx->timing) {
        char kbuf[64];
        snprintf(kbuf, sizeof(kbuf), "gemm_wres_kernel<%d, %d, %d>", WN, MODE, NT);
        kname = ssdseg_intern(kbuf);
    }
    SSDSEG_LAUNCH_NAMED(ctx, kname, c.bytes, c.flops, (gemm_wres_kernel<WN, MODE, NT>), grid, dim3(256), wres_lds_bytes(a.R, WN), a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// the gradient view of a backward-data call as the streamed operand
RowAArgs rowa_from_gview(const ssdseg_gview* dy, int ldy) {
    RowAArgs a{};
    a.a0 = dy->g; a.a1 = dy->y; a.cs = dy->scale; a.ct = dy->shift; a.ck1 = dy->k1; a.ck0 = dy->k0; a.act = dy->act; a.lda = ldy;
    return a;
}

// the same GEMM as the tile kernel takes it (wt: the forward wants the transposed weights, see launch_rowA)
template <int MODE>
PwTArgs pwt_from_rowa(const RowAArgs& a) {
    PwTArgs t{};
    t.a0 = a.a0; t.a1 = (MODE == 1 && a.cs != nullptr) ? a.a1 : a.a0;
    t.cs = a.cs; t.ct = a.ct; t.ck1 = a.ck1; t.ck0 = a.ck0; t.act = a.act; t.lda = a.lda;
    t.wt = a.b;
    t.out = a.out; t.ldo = a.ldo; t.residual = a.residual; t.ldr = a.ldr; t.accumulate = a.accumulate;
    t.stats = a.stats; t.M = a.I; t.cred = a.R; t.nout = a.J;
    t.bn_y = a.bn_y; t.ldby = a.ldby; t.bn_s = a.bn_s; t.bn_t = a.bn_t; t.bn_mean = a.bn_mean; t.bn_istd = a.bn_istd; t.bn_act = a.bn_act;
    t.bnpart = a.bnpart;
    return t;
}

// wt_pre (forward only, may be nullptr): the weights already transposed to [J][R] by ssdseg_transpose_batch
template <int MODE, int LD>
int launch_rowA(ssdseg_ctx* ctx, const RowAArgs& a, const float* wt_pre = nullptr) {
    int wn = (MODE == 1 && LD == 0) ? rowA_wn_bwd(a.I, a.J, a.R) : rowA_wn(a.I, a.J);
    const int nparts = rowA_grid_y(a.I, a.J);   // BN-statistics partial rows the caller allocated: fixed by (I, J) alone
    const bool adds = a.accumulate != 0 || a.residual != nullptr;
    // (the forward's residual / accumulate go to the rowA kernel whatever the switches say)
    if (LD == 0 && !(MODE == 0 && adds) && pw_tile_wanted(MODE, a.I, a.lda, a.R, a.J, false, adds)) {
        PwTArgs t = pwt_from_rowa<MODE>(a);
        if (MODE == 0 && wt_pre != nullptr) {
            t.wt = wt_pre;
        } else if (MODE == 0) {
            // the reduction channel must be contiguous in the staged weight rows: W[k][n] -> Wt[n][k] (one small transpose per call)
            void* ws;
            int rc = ssdseg_workspace(ctx, (size_t)a.R * a.J * sizeof(float), &ws);
            if (rc) return rc;
            rc = ssdseg_transpose_w(ctx, a.b, (float*)ws, a.R, a.J, 1);
            if (rc) return rc;
            t.wt = (const float*)ws;
        }
        return pw_tile_launch<MODE>(ctx, t, a.stats != nullptr ? nparts : 0, rowa_cost<MODE, 0, 0, 0>(a).view_bytes);
    }
    // Backward-data of the 30x40-stage expand convs (38400 rows = 300 row tiles, 384-576 reduction channels of a TWO-tensor
    // gradient view, 64-96 output columns): the default picks 32-column tiles to have 600-900 blocks, and every column tile
    // re-reads the whole (g, y) operand from the fabric (measured 5 TB/s of L2-level reads for 1.4 TB/s algorithmic).  One
    // column tile spanning all outputs reads it once; with >= 256 row tiles there is still a block per CU (109 -> 88 us).
    // Not for the 15x20 stage (75 row tiles: 2x slower) and no gain for the forward (single-tensor operand).
    int grid_y = (MODE == 1 && LD == 0) ? rowA_grid_y_wn(a.I, a.J, wn) : nparts;   // (no statistics table in backward-data: free choice)
    if (MODE == 1 && LD == 0 && a.cs != nullptr && a.R >= 256) {
        const int wide = cdiv(a.J, 32), mtiles = cdiv(a.I, BM);
        if (wide > wn && wide <= 3 && mtiles >= 256 && a.I < ROWA_OCC_ROWS) { wn = wide; grid_y = mtiles < 2048 ? mtiles : 2048; }
    }
    const dim3 grid(cdiv(a.J, 32 * wn), grid_y);
    if constexpr (LD == 0) {   // (the resident and float4-epilogue kernels exist for the plain pointwise GEMM only)
        // Measured per layer on MI355X (profiles/r01_wres_vs_general_per_layer.txt): the resident kernel wins when every wave
        // streams several row tiles (>= ~500k rows: the 240x320 and 120x160 stages at batch 32) and loses 10-30 % below that,
        // where its once-per-block weight load is not amortised; its 5-tile backward variant needs > 256 registers.
        // Same grid, same partial rows as the rowA kernel.
        if (wres_lds_bytes(a.R, wn) > 0 && (wres_mode() == 2 || (wres_mode() == 1 && a.I >= 500000 && !(MODE == 1 && wn >= 4))))
            return for_width<1, 5>(wn, [&](auto W) { return wres_launch_inst<decltype(W)::value, MODE, 0>(ctx, a, grid); });
        // wide, 16-byte-aligned outputs leave through the LDS-transposed float4 epilogue (16 B per lane instead of 4)
        if (wn >= 2 && !env_is("SSDSEG_NO_F4_EPILOGUE", '1') && a.J % 4 == 0 && a.ldo % 4 == 0 && ((uintptr_t)a.out & 15) == 0 &&
            (a.residual == nullptr || (a.ldr % 4 == 0 && ((uintptr_t)a.residual & 15) == 0)))
            return rowa_launch<MODE, 0, 1, 2>(ctx, a, wn, grid);
    }
    return rowa_launch<MODE, LD, 0, 1>(ctx, a, wn, grid);
}

// Wt[n][k] = W[k][n] for a whole table of matrices in ONE launch: blockIdx.y = matrix, blockIdx.x strides over its 32x32 tiles.
// table[mat] = {source pointer, destination pointer, k, n} as four 64-bit words.
__global__ void __launch_bounds__(256) transpose_batch_kernel(const long long* __restrict__ table) {
    __shared__ float tile[32][33];
    const long long* e = table + 4 * (long long)blockIdx.y;
    const float* __restrict__ w = reinterpret_cast<const float*>(e[0]);
    float* __restrict__ wt = reinterpret_cast<float*>(e[1]);
    const int k = (int)e[2], n = (int)e[3];
    const int tn = (n + 31) / 32, tk = (k + 31) / 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int t = blockIdx.x; t < tn * tk; t += gridDim.x) {
        const int c0 = (t / tn) * 32, n0 = (t % tn) * 32;
        for (int r = ty; r < 32; r += 8) {
            const int c = c0 + r, j = n0 + tx;
            tile[r][tx] = (c < k && j < n) ? w[(long long)c * n + j] : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int j = n0 + r, c = c0 + tx;
            if (j < n && c < k) wt[(long long)j * k + c] = tile[tx][r];
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

// ---- what conv3.hip and stem.hip take from this unit (gemm_internal.h): thin wrappers over the templates, so that every
// gemm_rowA_kernel instantiation stays in this unit
int ssdseg_rowA_grid_y(int rows, int cols) { return rowA_grid_y(rows, cols); }
int ssdseg_rowA_conv3_fwd(ssdseg_ctx* ctx, const ssdseg_rowa_args& a) { return launch_rowA<0, 1>(ctx, RowAArgs{a}); }
int ssdseg_rowA_conv3_bwd_data(ssdseg_ctx* ctx, const ssdseg_rowa_args& a) { return launch_rowA<1, 1>(ctx, RowAArgs{a}); }
int ssdseg_rowA_stem_fwd(ssdseg_ctx* ctx, const ssdseg_rowa_args& a) { return launch_rowA<0, 2>(ctx, RowAArgs{a}); }

int ssdseg_pwconv_parts(int m, int n, int* nparts_host) {
    SSDSEG_ARG(m > 0, 1);
    SSDSEG_ARG(n > 0, 2);
    SSDSEG_ARG(nparts_host != nullptr, 3);
    *nparts_host = rowA_grid_y(m, n);
    return 0;
}

int ssdseg_pwconv_fwd_wt(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, const float* wt, float* y, int ldy, int m,
                         int k, int n, float* stats) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= k && ldx % 4 == 0, 3);
    SSDSEG_ARG(w != nullptr, 4);
    SSDSEG_ARG(y != nullptr, 5);
    SSDSEG_ARG(ldy >= n, 6);
    SSDSEG_ARG(m > 0, 7);
    SSDSEG_ARG(k > 0 && k % 4 == 0, 8);
    SSDSEG_ARG(n > 0 && n % 4 == 0, 9);
    RowAArgs a{};
    a.a0 = in->x; a.cs = in->scale; a.ct = in->shift; a.act = in->act; a.lda = ldx;
    a.b = w; a.ldb = n;
    a.out = y; a.ldo = ldy;
    a.stats = stats;
    a.I = m; a.R = k; a.J = n;
    return launch_rowA<0, 0>(ctx, a, wt);
}

int ssdseg_pwconv_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int ldy, int m, int k,
                      int n, float* stats) {
    return ssdseg_pwconv_fwd_wt(ctx, in, ldx, w, nullptr, y, ldy, m, k, n, stats);
}

int ssdseg_pwconv_wt_floats(int m, int ldx, int k, int n, int* floats_host) {
    SSDSEG_ARG(m > 0, 1);
    SSDSEG_ARG(k > 0 && n > 0, 3);
    SSDSEG_ARG(floats_host != nullptr, 5);
    *floats_host = pw_tile_wanted(0, m, ldx, k, n, false, false) ? k * n : 0;
    return 0;
}

int ssdseg_transpose_batch(ssdseg_ctx* ctx, const long long* table, int nmat, int max_tiles, long long total_floats) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(table != nullptr, 2);
    SSDSEG_ARG(nmat > 0, 3);
    SSDSEG_ARG(max_tiles > 0, 4);
    const int gx = max_tiles < 64 ? max_tiles : 64;
    SSDSEG_LAUNCH(ctx, 8.0 * (double)total_floats, 0.0, transpose_batch_kernel, dim3(gx, nmat, 1), dim3(256), 0, table);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_pwconv_bwd_data(ssdseg_ctx* ctx, const ssdseg_gview* dy, int ldy, const float* w, float* dx, int ldx, int m,
                           int k, int n, const float* residual, int ldr, int accumulate) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 2);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 2);
    SSDSEG_ARG(ldy >= n && ldy % 4 == 0, 3);
    SSDSEG_ARG(w != nullptr, 4);
    SSDSEG_ARG(dx != nullptr, 5);
    SSDSEG_ARG(ldx >= k, 6);
    SSDSEG_ARG(m > 0, 7);
    SSDSEG_ARG(k > 0 && k % 4 == 0, 8);
    SSDSEG_ARG(n > 0 && n % 4 == 0, 9);
    SSDSEG_ARG(residual == nullptr || ldr >= k, 11);
    RowAArgs a = rowa_from_gview(dy, ldy);
    a.b = w; a.ldb = n;
    a.out = dx; a.ldo = ldx;
    a.residual = residual; a.ldr = ldr; a.accumulate = accumulate;
    a.I = m; a.R = n; a.J = k;
    return launch_rowA<1, 0>(ctx, a);
}

// dx and dW of a pointwise conv in ONE pass over the gradient (models.py:65-67 backward).  Shapes the fused kernel covers:
// k <= 32 input channels, n <= 192 output channels (MobileNetV2 expand convs of blocks 1-6, where the 6x-wide gradient
// is the whole cost); everything else runs the two separate kernels -- same results either way.
int ssdseg_pwconv_bwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy, const float* w, float* dx,
                      int lddx, float* dw, int m, int k, int n, const float* residual, int ldr, int accumulate) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(ldx >= k && ldx % 4 == 0, 3);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 4);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 4);
    SSDSEG_ARG(ldy >= n && ldy % 4 == 0, 5);
    SSDSEG_ARG(w != nullptr, 6);
    SSDSEG_ARG(dx != nullptr, 7);
    SSDSEG_ARG(lddx >= k, 8);
    SSDSEG_ARG(dw != nullptr, 9);
    SSDSEG_ARG(m > 0, 10);
    SSDSEG_ARG(k > 0 && k % 4 == 0, 11);
    SSDSEG_ARG(n > 0 && n % 4 == 0, 12);
    SSDSEG_ARG(residual == nullptr || ldr >= k, 14);
    // Measured per layer on MI355X (profiles/r01_wres_vs_general_per_layer.txt): the fused pass wins on the big early layers
    // (blocks 1-3 at batch 32: 760 -> 642, 492 -> 462, 456 -> 354 us against wgrad + bwd_data), is even at 153,600 rows and
    // loses with a single 32-column chunk, where the per-tile set-up dominates.  Its 16*NT accumulator registers cap the
    // occupancy at 1-2 waves per SIMD, which is why it stops at ~3.4 TB/s.  SSDSEG_PW_FUSED=1 forces it for every shape it
    // supports (k <= 32, n <= 192); the parity tests run both ways.
    // SSDSEG_PW_FUSED "1": every supported shape, "0": never, unset: where it measured faster
    const bool force_fused = env_is("SSDSEG_PW_FUSED", '1'), never_fused = env_is("SSDSEG_PW_FUSED", '0');
    const bool fused = !never_fused && k <= 32 && n <= 192 && (force_fused || (n > 32 && m >= 500000));
    if (!fused) {
        // dW is off the critical path (nothing reads it before the optimizer): it runs on the side stream, concurrently with
        // the backward-data GEMM and whatever follows it on the main stream
        const bool side = ssdseg_side_begin(ctx);
        int rc = ssdseg_pwconv_bwd_weight(ctx, in, ldx, dy, ldy, dw, m, k, n);
        if (side) ssdseg_side_end(ctx);
        if (rc) return rc;
        return ssdseg_pwconv_bwd_data(ctx, dy, ldy, w, dx, lddx, m, k, n, residual, ldr, accumulate);
    }
    RowAArgs a = rowa_from_gview(dy, ldy);
    a.b = w; a.ldb = n;
    a.out = dx; a.ldo = lddx;
    a.residual = residual; a.ldr = ldr; a.accumulate = accumulate;
    a.I = m; a.R = n; a.J = k;
    a.xw = in->x; a.xws = in->scale; a.xwt = in->shift; a.xwact = in->act; a.ldxw = ldx;
    const int mtiles = cdiv(m, BM);
    const int nt = cdiv(n, 32);   // NT > 0: fused dW, one accumulator tile per 32-column chunk of dy
    // two resident blocks per CU (112 + 16*NT registers each); every block walks >= 1 row tile.  (Round 3: three blocks per CU for
    // NT <= 3 -- 168 registers, 12 waves per CU -- left the block-1 expand backward at 0.642 ms: not short of waves in flight.)
    int gy = 2 * ctx->num_cus;
    if (gy > mtiles) gy = mtiles;
    void* ws;
    int rc = ssdseg_partials(ctx, (size_t)gy * k * n * sizeof(float), &ws);
    if (rc) return rc;
    a.wpart = (float*)ws;
    const dim3 grid(1, gy, 1);
    if (wres_enabled() && wres_lds_bytes(n, 1) > 0)
        rc = for_width<1, 6>(nt, [&](auto NT) { return wres_launch_inst<1, 1, decltype(NT)::value>(ctx, a, grid); });
    else
        rc = for_width_occ<1, 6>(nt, a.I >= occ_rows(), [&](auto NT, auto OCC) {
            return rowa_launch_inst<1, 1, 0, decltype(NT)::value, 0, decltype(OCC)::value>(ctx, a, grid);
        });
    if (rc) return rc;
    if (gy == 1) {
        SSDSEG_HIP(hipMemcpyAsync(dw, a.wpart, (size_t)k * n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    return ssdseg_colsum(ctx, a.wpart, gy, (long long)k * n, dw);
}

// dx = dy * w^T plus the BatchNormalization backward of the layer that feeds this conv (the depthwise BN in front of a project
// conv): the backward-data kernel's float4 epilogue reduces sum(mask*dx), sum(mask*dx*xhat) while it stores dx.  Only valid when
// this conv is the ONLY consumer of that BatchNorm's output.  Falls back to the separate reduction pass for tensors that are not 16-byte
// aligned (lddx is a multiple of 4: the callers check it).
// Shared by ssdseg_pwconv_bwd_bn and the tap-expanded form of the narrow 3x3 conv (ssdseg_conv3x3_bwd_data_bn).
int ssdseg_pwconv_bwd_data_bn(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy, const float* w, float* dx,
                              int lddx, int m, int k, int n, const float* in_mean, const float* in_invstd, float* in_dgamma,
                              float* in_dbeta, float* in_k1, float* in_k0) {
    int rc = 0;
    const bool aligned = lddx % 4 == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)in->x & 15) == 0;
    if (!aligned || env_is("SSDSEG_NO_BN_EPILOGUE", '1')) {
        rc = ssdseg_pwconv_bwd_data(ctx, dy, ldy, w, dx, lddx, m, k, n, nullptr, 0, 0);
        if (rc) return rc;
        return ssdseg_bn_bwd_reduce(ctx, dx, lddx, in->x, ldx, m, k, in->scale, in->shift, in_mean, in_invstd, in->act, in_dgamma, in_dbeta,
                                    in_k1, in_k0);
    }
    RowAArgs a = rowa_from_gview(dy, ldy);
    a.b = w; a.ldb = n;
    a.out = dx; a.ldo = lddx;
    a.I = m; a.R = n; a.J = k;
    a.bn_y = in->x; a.ldby = ldx; a.bn_s = in->scale; a.bn_t = in->shift; a.bn_mean = in_mean; a.bn_istd = in_invstd; a.bn_act = in->act;
    // the tile GEMM takes the BatchNorm-backward sums in its epilogue as well (pw_tile.h); either kernel writes `nparts` partial rows
    const bool tile = pw_tile_wanted(1, m, ldy, n, k, true, false);
    const int wn = rowA_wn_bwd(m, k, n);
    const int nparts = tile ? pwt_part_rows(m, m >= 65536 ? 256 : 128, 1) : rowA_grid_y_wn(m, k, wn);
    void* ws;
    rc = ssdseg_workspace(ctx, (size_t)nparts * 2 * k * sizeof(float), &ws);
    if (rc) return rc;
    a.bnpart = (float*)ws;
    if (tile) rc = pw_tile_launch<1>(ctx, pwt_from_rowa<1>(a), nparts, rowa_cost<1, 0, 0, 2>(a).view_bytes);
    else rc = rowa_launch<1, 0, 2, 1>(ctx, a, wn, dim3(cdiv(k, 32 * wn), nparts, 1));
    if (rc) return rc;
    return ssdseg_bn_bwd_finalize_launch(ctx, a.bnpart, nparts, k, (double)m, in->scale, in_mean, in_invstd, in_dgamma, in_dbeta, in_k1, in_k0);
}

int ssdseg_pwconv_bwd_bn(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy, const float* w, float* dx,
                         int lddx, float* dw, int m, int k, int n, const float* in_mean, const float* in_invstd, float* in_dgamma,
                         float* in_dbeta, float* in_k1, float* in_k0) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && in->scale != nullptr && in->shift != nullptr, 2);
    SSDSEG_ARG(ldx >= k && ldx % 4 == 0, 3);
    SSDSEG_ARG(dy != nullptr && dy->g != nullptr, 4);
    SSDSEG_ARG(dy->scale == nullptr || (dy->y && dy->shift && dy->k1 && dy->k0), 4);
    SSDSEG_ARG(ldy >= n && ldy % 4 == 0, 5);
    SSDSEG_ARG(w != nullptr, 6);
    SSDSEG_ARG(dx != nullptr, 7);
    // (a multiple of 4: the float4 epilogue stores dx rows as float4 and the fall-back's ssdseg_bn_bwd_reduce reads them back that way;
    // checked here, before the input-gradient GEMM is launched, not by that reduction after it)
    SSDSEG_ARG(lddx >= k && lddx % 4 == 0, 8);
    SSDSEG_ARG(dw != nullptr, 9);
    SSDSEG_ARG(m > 0, 10);
    SSDSEG_ARG(k > 0 && k % 4 == 0, 11);
    SSDSEG_ARG(n > 0 && n % 4 == 0, 12);
    SSDSEG_ARG(in_mean != nullptr && in_invstd != nullptr, 13);
    SSDSEG_ARG(in_k1 != nullptr && in_k0 != nullptr, 17);
    // dW first, on the side stream (it only reads)
    const bool side = ssdseg_side_begin(ctx);
    int rc = ssdseg_pwconv_bwd_weight(ctx, in, ldx, dy, ldy, dw, m, k, n);
    if (side) ssdseg_side_end(ctx);
    if (rc) return rc;
    return ssdseg_pwconv_bwd_data_bn(ctx, in, ldx, dy, ldy, w, dx, lddx, m, k, n, in_mean, in_invstd, in_dgamma, in_dbeta, in_k1, in_k0);
}


}  // extern "C"
