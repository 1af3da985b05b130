// Dense 3x3 stride-1 SAME convolution (DeepLabV3+ decoder, reference blocks.py:117-127): every form of it and the ssdseg_conv3x3_*
// entry points that choose between them.
//   narrow (cout <= 8)      tap-expanded columns around the pointwise GEMMs of gemm.hip (this file); conv3n.hip: the direct input gradient
//   halo tile               conv3_tile.h (forward, input gradient), conv3_wgrad_tile.h (weight gradient)
//   Winograd F(2x2, 3x3)    conv3_wino.h, conv3_wino_wgrad.h          F(4x4, 3x3)   conv3_wino4.h
//   nine taps in one pass   conv3_wgrad.h (weight gradient with a BatchNorm gradient view)
//   implicit GEMM           gemm_rowA_kernel<.., LD = 1> / gemm_wgrad_kernel per tap in gemm.hip, reached through gemm_internal.h
// Host side, top to bottom: the narrow form's kernels and scratch; the PLAN of a call (Conv3Plan: which family runs a layer, decided
// once per call by conv3_fwd_plan / conv3_bwd_data_plan / conv3_wgrad_plan from the shape, the row stride, the operand form and the
// switches); one launch function per family, each taking the plan and the call's operands; the entry points, which check their
// arguments, make the plan, zero the statistics rows the planned kernel leaves and switch on plan.family.
#include "gemm_internal.h"
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
// the hold on a Conv3nScratch for the scope of a nested pointwise call: no return path leaves the reservation behind
struct Conv3nHold {
    ssdseg_ctx* ctx;
    size_t bytes;
    Conv3nHold(ssdseg_ctx* c, const Conv3nScratch& s) : ctx(c), bytes(s.bytes) { ctx->ws_reserved += bytes; }
    ~Conv3nHold() { ctx->ws_reserved -= bytes; }
};

// ------------------------------------------------------------------------------------------------ the plan of a call
// Everything the host decides about one call, decided ONCE: the kernel family, that family's geometry, the BatchNorm statistics
// rows it writes and the split-K of a weight gradient.  ssdseg_conv3x3_parts, the zeroing of surplus statistics rows,
// ssdseg_conv3x3_saved_floats, the saved-input pair and the launches all read it.  The switches are read on every
// call, not cached: the parity tests flip them between calls.  What the switches do that their names do not say:
//   - SSDSEG_CONV3_TILE=0 turns the Winograd forms off too (forward, input gradient AND weight gradient);
//   - ANY value of SSDSEG_CONV3_WGRAD or SSDSEG_CONV3_SAVED, not only "0", turns the saved-input pair off; any value of _WGRAD turns
//     the Winograd and halo-tile weight gradients off, "taps" alone the nine-tap kernels;
//   - the input gradient asks the tiled families with cin and cout swapped (it reduces over cout and produces cin);
//   - the F(4x4) form takes only layers the F(2x2) form takes, and its fit test includes the F(2x2) form's LDS bound.
enum Conv3Family {
    C3_NARROW,          // tap-expanded columns around the pointwise GEMMs
    C3_NARROW_DIRECT,   // input gradient + BatchNorm sums of the 256 -> 4 conv as one streaming kernel (conv3n.hip)
    C3_TILE,            // halo tiles
    C3_WINO,            // Winograd F(2x2, 3x3)
    C3_WINO4,           // Winograd F(4x4, 3x3)
    C3_GEMM,            // implicit GEMM
    // weight gradient; C3W_NINE: nine taps in one pass (conv3_wgrad12_kernel, conv3_wgrad9_kernel<4> or <1>: Conv3Plan::nine), C3W_TAPS: a GEMM per tap
    C3W_NARROW, C3W_WINO, C3W_TILE, C3W_NINE, C3W_TAPS
};
enum { C3_WGRAD_UNSET, C3_WGRAD_TAPS, C3_WGRAD_NINE, C3_WGRAD_OTHER };
struct Conv3Switches { bool narrow, tile, saved; int wino, f4, wgrad; };
Conv3Switches conv3_switches() {
    Conv3Switches s;
    s.narrow = !env_is("SSDSEG_CONV3_NARROW", '0');      // "0": the implicit-GEMM kernels (A/B measurements, parity tests)
    s.tile = !env_is("SSDSEG_CONV3_TILE", '0');          // likewise
    // 0 off, 1 forced (any size; parity tests), 2 automatic (unset or empty)
    s.wino = !s.tile || env_is("SSDSEG_CONV3_WINOGRAD", '0') ? 0 : (!env_set("SSDSEG_CONV3_WINOGRAD") || env_is("SSDSEG_CONV3_WINOGRAD", '\0') ? 2 : 1);
    s.f4 = env_is("SSDSEG_CONV3_F4", '0') ? 0 : (env_is("SSDSEG_CONV3_F4", '1') ? 1 : 2);      // never, wherever it fits (parity tests), automatic
    // "taps": the nine shifted GEMMs, "nine": the nine-wave kernel for every tile width (A/B measurements, parity tests)
    const int pick = env_pick("SSDSEG_CONV3_WGRAD", {"taps", "nine"});
    s.wgrad = pick != 0 ? pick : (env_set("SSDSEG_CONV3_WGRAD") ? C3_WGRAD_OTHER : C3_WGRAD_UNSET);
    s.saved = !env_set("SSDSEG_CONV3_SAVED");
    return s;
}

struct Conv3TGeom { int tiles_h, tiles_w, mtiles, ntiles_n, ncols, wn; };
struct Wino4Geom { int tr, tc, trs, tiles_h, tiles_w; };
struct Conv3Plan {
    Conv3Family family;
    Conv3TGeom tg;                  // C3_TILE; C3_WINO (the pixel tiles: its column tiles are WINO_NT wide)
    Wino4Geom g4;                   // C3_WINO4
    int rows;                       // forward: partial rows of the BatchNorm statistics table the kernel writes
    int nine;                       // C3W_NINE: 12 = the 12-wave kernel, 4 / 1 = conv3_wgrad9_kernel<4> / <1>
    int gx, gy;                     // C3W_TILE: gx (k, n) tiles;  C3W_NINE: gx x gy of them
    long long steps, splits, steps_per_split;      // C3W_TILE, C3W_NINE: split-K over the pixel steps
};

bool conv3_narrow(const Conv3Switches& sw, int cin, int cout) { return sw.narrow && cout <= C3N_MAX_COUT && cin >= 4 * cout; }
// 32-bit buffer offsets: the streamed tensor (row stride ld) has to stay below 2^31 bytes
bool conv3_tile_fits(int n, int h, int w, int ld) { return (long long)n * h * w * ld * 4 < (1LL << 31); }

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
// Winograd F(2x2): automatic where the 16 transformed GEMMs fill the chip -- >= 64 output channels, a few hundred pixel tiles
bool conv3_wino_takes(const Conv3Switches& sw, int n, int h, int w, int cred, int nout) {
    if (sw.wino == 0 || cred % C3T_KC != 0 || wino_lds_floats(cred) * sizeof(float) > (size_t)160 * 1024) return false;
    return sw.wino == 1 || (nout >= 64 && (long long)n * cdiv(h, C3T_ROWS) * cdiv(w, C3T_COLS) >= 256);
}
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
// F(4x4), of the layers the F(2x2) form takes: automatic where every CU gets a few work items (pixel tile x 32-channel tile) -- the
// decoder conv of the full-size models
bool conv3_wino4_takes(const Conv3Switches& sw, int n, int h, int w, int cred, int nout, Wino4Geom* g) {
    if (sw.f4 == 0 || !wino4_fits(h, w, cred, nout, g)) return false;
    return sw.f4 == 1 || (long long)n * g->tiles_h * g->tiles_w * cdiv(nout, W4_NT) >= 2048;
}

// The families that stream halo tiles of a tensor with `cred` channels at row stride `ld` and produce `nout` channels: the forward
// over (x, cin -> cout), the input gradient over (dy, cout -> cin).  false: none of them takes the layer.
bool conv3_tiled_plan(const Conv3Switches& sw, int n, int h, int w, int ld, int cred, int nout, Conv3Plan* p) {
    if (!sw.tile || cred % C3T_KC != 0 || !conv3_tile_fits(n, h, w, ld)) return false;
    p->tg = conv3t_geometry(n, h, w, nout);
    p->rows = p->tg.mtiles;                  // halo tiles and F(2x2) share the pixel tiles: one row per 8 x 32 tile
    if (!conv3_wino_takes(sw, n, h, w, cred, nout)) p->family = C3_TILE;
    else if (!conv3_wino4_takes(sw, n, h, w, cred, nout, &p->g4)) p->family = C3_WINO;
    else {
        p->family = C3_WINO4;
        p->rows = n * p->g4.tiles_h * p->g4.tiles_w;      // one row per block of 4x4-pixel tiles
    }
    return true;
}

// WHICH FORWARD KERNEL RUNS THIS LAYER.  ldx: row stride of the tensor the kernel streams (the saved-input forward streams its dense
// zero-bordered copy: ldx = cin there, whatever the layer's input has)
Conv3Plan conv3_fwd_plan(const Conv3Switches& sw, int n, int h, int w, int ldx, int cin, int cout) {
    Conv3Plan p{};
    if (conv3_narrow(sw, cin, cout)) p.family = C3_NARROW;
    else if (conv3_tiled_plan(sw, n, h, w, ldx, cin, cout, &p)) return p;
    else p.family = C3_GEMM;
    p.rows = ssdseg_rowA_grid_y(n * h * w, cout);      // the tap-expanded form sums its taps on the implicit GEMM's row grid
    return p;
}
// rows of the BatchNorm statistics table of a layer: the largest count among the forward kernels that can take it, whatever the
// switches say when the table is allocated
int conv3_fwd_table_rows(int n, int h, int w, int cin, int cout) {
    int rows = ssdseg_rowA_grid_y(n * h * w, cout);
    if (cin % C3T_KC != 0) return rows;
    const int tiles = conv3t_geometry(n, h, w, cout).mtiles;
    if (tiles > rows) rows = tiles;
    Wino4Geom g;
    if (wino4_fits(h, w, cin, cout, &g) && n * g.tiles_h * g.tiles_w > rows) rows = n * g.tiles_h * g.tiles_w;
    return rows;
}

// WHICH INPUT-GRADIENT KERNEL RUNS THIS LAYER.  gview_bn: the gradient comes as a BatchNorm gradient view (the tiled families read a
// plain tensor: nine taps would each re-form the view -- ssdseg_gview_materialize);  in_bn: the call also wants the BatchNorm sums
// of the layer's input (ssdseg_conv3x3_bwd_data_bn)
Conv3Plan conv3_bwd_data_plan(const Conv3Switches& sw, int n, int h, int w, int ldx, int cin, int cout, bool gview_bn, bool in_bn) {
    Conv3Plan p{};
    if (conv3_narrow(sw, cin, cout))
        p.family = in_bn && ssdseg_conv3n_direct_takes(cin, cout, ldx) && (long long)n * h * w < (1LL << 29) ? C3_NARROW_DIRECT : C3_NARROW;
    else if (gview_bn || !conv3_tiled_plan(sw, n, h, w, cout, cout, cin, &p)) p.family = C3_GEMM;
    return p;
}

// weight gradient in the Winograd form (conv3_wino_wgrad.h): h and w even, everything below 2^31 bytes
bool conv3_wino_wgrad_takes(const Conv3Switches& sw, int n, int h, int w, int cin, int cout) {
    if (sw.wino == 0 || h % 2 != 0 || w % 2 != 0) return false;
    if ((long long)n * (h + 2) * (w + 2) * cin * 4 >= (1LL << 31) || (long long)n * h * w * cout * 4 >= (1LL << 31)) return false;
    return sw.wino == 1 || (long long)n * (h / 2) * cdiv(w, 32) >= 512;
}
// split-K of a weight gradient over p->steps reduction steps: as many splits as `want` asks for while each keeps >= min_steps steps,
// dealt evenly (no empty split)
void conv3_wgrad_splits(Conv3Plan* p, long long want, int min_steps) {
    long long splits = want;
    if (splits > p->steps / min_steps) splits = p->steps / min_steps;
    if (splits < 1) splits = 1;
    p->steps_per_split = (p->steps + splits - 1) / splits;
    p->splits = (p->steps + p->steps_per_split - 1) / p->steps_per_split;
}
// WHICH WEIGHT-GRADIENT KERNEL RUNS THIS LAYER
Conv3Family conv3_wgrad_family(const Conv3Switches& sw, int n, int h, int w, int ldx, int cin, int cout, bool gview_bn) {
    const bool plain = sw.wgrad == C3_WGRAD_UNSET && !gview_bn;
    if (conv3_narrow(sw, cin, cout)) return C3W_NARROW;
    if (plain && conv3_wino_wgrad_takes(sw, n, h, w, cin, cout)) return C3W_WINO;
    if (plain && sw.tile && conv3_tile_fits(n, h, w, ldx) && conv3_tile_fits(n, h, w, cout)) return C3W_TILE;
    return sw.wgrad != C3_WGRAD_TAPS ? C3W_NINE : C3W_TAPS;
}
Conv3Plan conv3_wgrad_plan(const Conv3Switches& sw, int num_cus, int n, int h, int w, int ldx, int cin, int cout, bool gview_bn) {
    Conv3Plan p{};
    p.family = conv3_wgrad_family(sw, n, h, w, ldx, cin, cout, gview_bn);
    if (p.family == C3W_TILE) {
        // 64 x 64 (k, n) tiles of all nine taps, one image row x 32 columns per step; two blocks per CU (67 KB of LDS, <= 256 registers each)
        p.gx = cdiv(cin, W3T_KT) * cdiv(cout, W3T_NT);
        p.steps = n * cdiv(w, W3T_COLS) * h;
        conv3_wgrad_splits(&p, 2 * num_cus / p.gx, 4);
    } else if (p.family == C3W_NINE) {
        const int wn = cout > 32 ? 4 : 1;
        p.nine = wn == 4 && sw.wgrad != C3_WGRAD_NINE ? 12 : wn;
        p.gx = cdiv(cout, 32 * wn);
        p.gy = cdiv(cin, C9_KT);
        p.steps = (long long)n * h * cdiv(w, C9_PX);
        conv3_wgrad_splits(&p, (2LL * num_cus) / ((long long)p.gx * p.gy), 8);
    }
    return p;
}

// the saved-input pair (include/ssdseg.h) exists where the forward over the dense saved copy AND the weight gradient are both in
// the Winograd form, with neither SSDSEG_CONV3_WGRAD nor SSDSEG_CONV3_SAVED set
bool conv3_saved_pair(const Conv3Switches& sw, int n, int h, int w, int cin, int cout) {
    const Conv3Family fwd = conv3_fwd_plan(sw, n, h, w, cin, cin, cout).family;
    return sw.saved && (fwd == C3_WINO || fwd == C3_WINO4) && conv3_wgrad_family(sw, n, h, w, cin, cin, cout, false) == C3W_WINO;
}

// ------------------------------------------------------------------------------------------------ launches, one per family
// what an entry point hands to its family's launch function
struct Conv3BnOut { const float *mean, *invstd; float *dgamma, *dbeta, *k1, *k0; };
struct Conv3Call {
    int n, h, w, cin, cout;
    const ssdseg_view* in;      // the layer's input view: forward, weight gradient, input gradient with BatchNorm sums
    int ldx;                    // row stride of the input, and of dx
    const ssdseg_gview* dy;     // backward
    const float* wgt;
    float* out;                 // y | dx | dw
    float* stats;               // forward
    int accumulate;             // input gradient
    const Conv3BnOut* bn;       // input gradient with BatchNorm sums
};

// X + Y + W (backward: dY + dX + W, X + dY + dW) of a conv over m pixels
double conv3_cost_bytes(double m, int cred, int nout) { return 4.0 * (m * cred + m * nout + 9.0 * cred * nout); }

// the input-view / gradient-view fields, which the argument structs of the weight-gradient kernels and GEMMs name alike
template <typename Args>
void conv3_set_view(Args* a, const ssdseg_view* in, int ldx) {
    a->x = in->x; a->xs = in->scale; a->xt = in->shift; a->xact = in->act; a->ldx = ldx;
}
template <typename Args>
void conv3_set_gview(Args* a, const ssdseg_gview* dy) {
    a->g = dy->g; a->y = dy->y; a->gs = dy->scale; a->gt = dy->shift; a->gk1 = dy->k1; a->gk0 = dy->k0; a->gact = dy->act;
}

// out[n][h + 2][w + 2][cin] = the zero-bordered activated input, channels c_from .. cin - 1 of it
int conv3_pad_view(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, float* out, int n, int h, int w, int cin, int c_from) {
    const long long tot4 = (long long)n * (h + 2) * (w + 2) * ((cin - c_from) / 4);
    SSDSEG_LAUNCH(ctx, 8.0 * n * h * w * (cin - c_from), 0.0, conv3_pad_view_kernel, dim3((unsigned)((tot4 + 255) / 256 < 16384 ? (tot4 + 255) / 256 : 16384)), dim3(256), 0,
                  in->x, in->scale, in->shift, in->act, ldx, out, n, h, w, cin, c_from);
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

// ---- narrow form
// w != nullptr: also packs the weights into W2
int conv3n_reserve(ssdseg_ctx* ctx, const float* w, const Conv3Call& c, Conv3nScratch* s) {
    s->m = (long long)c.n * c.h * c.w;
    s->nc = 9 * c.cout; s->cv = c.cout / 4;
    const size_t wb = align256((size_t)c.cin * s->nc * sizeof(float)), zb = align256((size_t)s->m * s->nc * sizeof(float));
    s->bytes = wb + zb;
    void* ws;
    int rc = ssdseg_workspace(ctx, s->bytes + s->bytes / 2 + ((size_t)64 << 20), &ws);
    if (rc) return rc;
    s->w2 = (float*)ws;
    s->z = (float*)((char*)ws + wb);
    if (w == nullptr) return 0;
    SSDSEG_LAUNCH(ctx, 8.0 * 9 * c.cin * c.cout, 0.0, conv3n_pack_w_kernel, dim3(cdiv(9 * c.cin * c.cout, 256)), dim3(256), 0, w, s->w2, c.cin, c.cout, 0);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
// s.z = dz[m][tap][o] = dy[m - d(tap)][o], dy formed from the gradient view on the way
int conv3n_shift(ssdseg_ctx* ctx, const Conv3Call& c, const Conv3nScratch& s) {
    const long long tot = s.m * 9 * s.cv;
    SSDSEG_ARG(tot < (1LL << 31), 6);       // 32-bit element indices in conv3n_shift_kernel
    SSDSEG_LAUNCH(ctx, 4.0 * s.m * (s.nc + (c.dy->scale ? 2.0 : 1.0) * c.cout), 0.0, conv3n_shift_kernel, dim3((unsigned)((tot + 255) / 256 < 8192 ? (tot + 255) / 256 : 8192)),
                  dim3(256), 0, c.dy->g, c.dy->y, c.dy->scale, c.dy->shift, c.dy->k1, c.dy->k0, c.dy->act, s.z, c.n, c.h, c.w, s.cv);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
int conv3n_fwd_launch(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv3Call& c) {
    Conv3nScratch s;
    int rc = conv3n_reserve(ctx, c.wgt, c, &s);
    if (rc) return rc;
    {
        Conv3nHold hold(ctx, s);
        rc = ssdseg_pwconv_fwd(ctx, c.in, c.ldx, s.w2, s.z, s.nc, (int)s.m, c.cin, s.nc, nullptr);
    }
    if (rc) return rc;
    SSDSEG_ARG((long long)s.m * s.cv < (1LL << 31), 6);   // 32-bit element indices in conv3n_tapsum_kernel
    const int blocks = c.stats != nullptr ? p.rows : (int)((s.m * s.cv + 255) / 256 < 4096 ? (s.m * s.cv + 255) / 256 : 4096);
    SSDSEG_LAUNCH(ctx, 4.0 * s.m * (s.nc + c.cout), 0.0, conv3n_tapsum_kernel, dim3(blocks), dim3(256), 0, (const float*)s.z, c.out, c.n, c.h, c.w, s.cv, c.stats);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
// input gradient in the tap-expanded form: dz[m][tap][o] = dy[m - d(tap)][o], then dx = dz * W2^T is a pointwise GEMM.  c.bn != nullptr:
// the GEMM's float4 epilogue holds the dx tile and reads the matching tile of the raw input -- that BN's sums ride there (the 256 -> 4
// logits conv of the decoder: one pass over the 614,400 x 256 gradient and its raw tensor less)
int conv3n_bwd_data_launch(ssdseg_ctx* ctx, const Conv3Call& c) {
    Conv3nScratch s;
    int rc = conv3n_reserve(ctx, c.wgt, c, &s);
    if (rc) return rc;
    rc = conv3n_shift(ctx, c, s);
    if (rc) return rc;
    ssdseg_gview idv{};
    idv.g = s.z;
    Conv3nHold hold(ctx, s);
    const Conv3BnOut* b = c.bn;
    if (b != nullptr) return ssdseg_pwconv_bwd_data_bn(ctx, c.in, c.ldx, &idv, s.nc, s.w2, c.out, c.ldx, (int)s.m, c.cin, s.nc, b->mean, b->invstd, b->dgamma, b->dbeta, b->k1, b->k0);
    return ssdseg_pwconv_bwd_data(ctx, &idv, s.nc, s.w2, c.out, c.ldx, (int)s.m, c.cin, s.nc, nullptr, 0, c.accumulate);
}
int conv3n_wgrad_launch(ssdseg_ctx* ctx, const Conv3Call& c) {
    Conv3nScratch s;      // (s.w2 holds dW2 here)
    int rc = conv3n_reserve(ctx, nullptr, c, &s);
    if (rc) return rc;
    rc = conv3n_shift(ctx, c, s);
    if (rc) return rc;
    ssdseg_wgrad_args a{};
    conv3_set_view(&a, c.in, c.ldx);
    a.g = s.z; a.ldy = s.nc;
    a.M = (int)s.m; a.K = c.cin; a.N = s.nc;
    {
        Conv3nHold hold(ctx, s);
        ssdseg_defer_hold(ctx, +1);           // dW2 is scratch, repacked right below: its column sum cannot wait for the flush
        rc = ssdseg_wgrad_run(ctx, a, s.w2);
        ssdseg_defer_hold(ctx, -1);
    }
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, 8.0 * 9 * c.cin * c.cout, 0.0, conv3n_pack_w_kernel, dim3(cdiv(9 * c.cin * c.cout, 256)), dim3(256), 0, (const float*)c.out, s.w2, c.cin, c.cout, 1);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// ---- the tiled families (forward: mode 0, input gradient: mode 1).  An entry point fills in / view / out / stats / shape of a
// Conv3TArgs; the launch functions add the weights, the tiling and the buffer extents.  w = the layer's [3][3][cin][cout] weights.
Conv3TArgs conv3t_args(const float* x, const float* cs, const float* ct, int act, int ldi, float* out, int ldo, int accumulate, float* stats, int n,
                       int h, int w, int cred, int nout) {
    Conv3TArgs t{};
    t.in = x; t.cs = cs; t.ct = ct; t.act = act; t.ldi = ldi;
    t.out = out; t.ldo = ldo; t.accumulate = accumulate;
    t.stats = stats;
    t.n = n; t.h = h; t.w = w; t.cred = cred; t.nout = nout;
    return t;
}
const char* conv3_role(int mode) { return mode ? "bwd_data" : "fwd"; }

// KERNEL<true> where the streamed tensor carries a view (BatchNorm coefficients or an activation), KERNEL<false> for a plain tensor.
// Registry name: the symbol as rocprofv3 spells it + the role.
template <auto WITH_VIEW, auto PLAIN, typename Args>
int conv3_viewed_launch(ssdseg_ctx* ctx, const char* symbol, int mode, double cost_bytes, double cost_flops, unsigned blocks, unsigned threads, size_t lds,
                        const Args& a) {
    int rc;
    if ((rc = conv3_announce_lds<PLAIN>(lds)) || (rc = conv3_announce_lds<WITH_VIEW>(lds))) return rc;
    const bool with_view = a.cs != nullptr || a.act != SSDSEG_ACT_NONE;
    char kbuf[64];
    snprintf(kbuf, sizeof(kbuf), "%s<%s> [%s]", symbol, with_view ? "true" : "false", conv3_role(mode));
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    if (with_view) SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, WITH_VIEW, dim3(blocks), dim3(threads), lds, a);
    else SSDSEG_LAUNCH_NAMED(ctx, kname, cost_bytes, cost_flops, PLAIN, dim3(blocks), dim3(threads), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

template <int WN>
int conv3_tile_launch_wn(ssdseg_ctx* ctx, const Conv3TArgs& a, const Conv3TGeom& g) {
    const size_t lds = conv3t_lds_floats(WN, a.cred) * sizeof(float);
    if (int rc = conv3_announce_lds<&conv3_tile_kernel<WN>>(lds)) return rc;
    char kbuf[64];
    snprintf(kbuf, sizeof(kbuf), "conv3_tile_kernel<%d> [%s]", WN, conv3_role(a.flip));
    const char* kname = ctx->timing ? ssdseg_intern(kbuf) : "";
    const double m = (double)a.n * a.h * a.w;
    SSDSEG_LAUNCH_NAMED(ctx, kname, conv3_cost_bytes(m, a.cred, a.nout), 18.0 * m * a.cred * a.nout, (conv3_tile_kernel<WN>), dim3((unsigned)(g.mtiles * g.ntiles_n)),
                        dim3(C3T_THREADS), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
int conv3_tile_launch(ssdseg_ctx* ctx, const Conv3Plan& p, Conv3TArgs a, const float* w, int cin, int cout, int mode) {
    if (mode == 0) {
        // weights with the reduction channel contiguous: W[tap][c][n] -> Wt[tap][n][c] (2.8 MB for the decoder conv, ~3 us)
        void* ws;
        int rc = ssdseg_workspace(ctx, (size_t)9 * cin * cout * sizeof(float), &ws);
        if (rc) return rc;
        rc = ssdseg_transpose_w(ctx, w, (float*)ws, cin, cout, 9);
        if (rc) return rc;
        a.wt = (const float*)ws;
    } else {
        // dx[p][c] = sum_{tap, n} dy[p - d(tap)][n] W[tap][c][n]: the forward loop over the mirrored taps; W's native layout already has
        // the reduction channel (n) contiguous
        a.wt = w;
        a.flip = 1;
    }
    const Conv3TGeom& g = p.tg;
    a.tiles_h = g.tiles_h; a.tiles_w = g.tiles_w; a.ntiles_n = g.ntiles_n; a.ncols = g.ncols;
    a.in_bytes = (unsigned)((((long long)a.n * a.h * a.w - 1) * a.ldi + a.cred) * 4);
    a.wt_bytes = (unsigned)((long long)9 * a.nout * a.cred * 4);
    return for_width<1, 5>(g.wn, [&](auto WN) { return conv3_tile_launch_wn<decltype(WN)::value>(ctx, a, g); });
}

int conv3_wino_launch(ssdseg_ctx* ctx, const Conv3Plan& p, Conv3TArgs a, const float* w, int cin, int cout, int mode) {
    void* ws;
    const int npad = cdiv(a.nout, WINO_NT) * WINO_NT;
    const size_t ubytes = (size_t)16 * a.cred * npad * sizeof(float);      // U[cred / 8][16][npad][8]
    int rc = ssdseg_workspace(ctx, ubytes, &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, 4.0 * (9 + 16) * cin * cout, 0.0, conv3_wino_weights_kernel, dim3(cdiv(cout, 32), cdiv(cin, 32)), dim3(256), 0, w, (float*)ws, cin, cout, mode);
    SSDSEG_LAUNCH_CHECK();
    a.wt = (const float*)ws;
    a.tiles_h = p.tg.tiles_h; a.tiles_w = p.tg.tiles_w; a.ntiles_n = cdiv(a.nout, WINO_NT); a.ncols = WINO_NT;
    if (a.in_hp == 0) { a.in_hp = a.h; a.in_wp = a.w; }
    // (the zero-bordered copy is entered at its pixel (1, 1): the last byte the kernel may touch is that of image pixel (h-1, w-1))
    a.in_bytes = (unsigned)(((((long long)(a.n - 1) * a.in_hp + a.h - 1) * a.in_wp + a.w - 1) * a.ldi + a.cred) * 4);
    a.wt_bytes = (unsigned)ubytes;
    const double m = (double)a.n * a.h * a.w;
    // flops EXECUTED on the MFMA pipe: 16 positions x (m / 4) tiles x 2 cred nout = 8 m cred nout -- 16/36 of the direct convolution's
    // 18 m cred nout (bench.py reports that figure beside it as `direct_equivalent`; the roofline fraction uses the executed ones)
    return conv3_viewed_launch<&conv3_wino_kernel<true>, &conv3_wino_kernel<false>>(ctx, "conv3_wino_kernel", mode, conv3_cost_bytes(m, a.cred, a.nout), 8.0 * m * a.cred * a.nout,
                                                                                   (unsigned)(p.tg.mtiles * a.ntiles_n), C3T_THREADS, wino_lds_floats(a.cred) * sizeof(float), a);
}

// the F(4x4) kernel's arguments from what the tiled families share: the tiling of g, the transformed weights u[cred / 8][36][npad][8]
Wino4Args wino4_args(const Conv3TArgs& a, const Wino4Geom& g, const float* u, int npad, size_t ubytes) {
    Wino4Args p{};
    p.in = a.in; p.cs = a.cs; p.ct = a.ct; p.act = a.act; p.ldi = a.ldi;
    p.u = u;
    p.out = a.out; p.ldo = a.ldo; p.accumulate = a.accumulate; p.stats = a.stats;
    p.n = a.n; p.h = a.h; p.w = a.w; p.cred = a.cred; p.nout = a.nout; p.npad = npad;
    p.tr = g.tr; p.tc = g.tc; p.trs = g.trs;
    p.qps = g.tr * g.trs;
    while ((p.qps & 15) != 1) ++p.qps;
    p.tiles_h = g.tiles_h; p.tiles_w = g.tiles_w; p.ntiles_n = npad / W4_NT;
    p.in_hp = a.in_hp ? a.in_hp : a.h; p.in_wp = a.in_hp ? a.in_wp : a.w;
    p.in_bytes = (unsigned)(((((long long)(a.n - 1) * p.in_hp + a.h - 1) * p.in_wp + a.w - 1) * a.ldi + a.cred) * 4);
    p.u_bytes = (unsigned)ubytes;
    const long long ob = (((long long)a.n * a.h * a.w - 1) * a.ldo + a.nout) * 4;
    p.out_bytes = ob < (1LL << 31) ? (unsigned)ob : 0u;
    // 32-bit buffer offsets do not reach: plain stores; SSDSEG_W4_PLAIN_STORES=1 (parity tests): that path at any size
    if ((ob >= (1LL << 31) || env_is("SSDSEG_W4_PLAIN_STORES", '1')) && !p.accumulate) p.accumulate = 2;
    p.group = (int)env_int("SSDSEG_W4_GROUP", 2);      // (A/B runs) channel tiles per group of the work order
    if (p.group < 1 || p.ntiles_n % p.group != 0) p.group = 1;
    p.trace = nullptr;
    return p;
}
int wino4_trace_report(ssdseg_ctx* ctx, unsigned long long* trace, int nblocks, long long items, int cred);

int conv3_wino4_launch(ssdseg_ctx* ctx, const Conv3Plan& plan, const Conv3TArgs& a, const float* w, int cin, int cout, int mode) {
    void* ws;
    const int npad = cdiv(a.nout, W4_NT) * W4_NT;
    const size_t ubytes = (size_t)36 * a.cred * npad * sizeof(float);      // U[cred / 8][36][npad][8]
    int rc = ssdseg_workspace(ctx, ubytes, &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, 4.0 * (9 + 36) * cin * cout, 0.0, conv3_wino4_weights_kernel, dim3(cdiv(cout, 32), cdiv(cin, 32)), dim3(256), 0, w, (float*)ws, cin, cout, mode);
    SSDSEG_LAUNCH_CHECK();
    Wino4Args p = wino4_args(a, plan.g4, (const float*)ws, npad, ubytes);
    // persistent blocks: one per CU (154 KB of LDS each), a multiple of 8 so that every XCD walks one contiguous run of the items
    const long long items = (long long)a.n * plan.g4.tiles_h * plan.g4.tiles_w * p.ntiles_n;
    int nblocks = ctx->num_cus;
    if (env_int("SSDSEG_W4_BLOCKS", 0) > 0) nblocks = (int)env_int("SSDSEG_W4_BLOCKS", 0);
    if (nblocks > items) nblocks = (int)items;
    if (nblocks >= 8 && items % 8 == 0) nblocks -= nblocks % 8;
    // (measurement only) per-item clocks of every block, read out below
    if (env_set("SSDSEG_W4_TRACE")) { SSDSEG_HIP(hipMalloc((void**)&p.trace, (size_t)nblocks * 64 * 4 * 8)); SSDSEG_HIP(hipMemset(p.trace, 0, (size_t)nblocks * 64 * 4 * 8)); }
    const double m = (double)a.n * a.h * a.w;
    // flops EXECUTED on the MFMA pipe: 36 positions x (m / 16) tiles x 2 cred nout = 4.5 m cred nout -- a quarter of the direct sum's 18
    rc = conv3_viewed_launch<&conv3_wino4_kernel<true>, &conv3_wino4_kernel<false>>(ctx, "conv3_wino4_kernel", mode, conv3_cost_bytes(m, a.cred, a.nout), 4.5 * m * a.cred * a.nout,
                                                                                   (unsigned)nblocks, W4_THREADS, wino4_lds_floats(a.cred) * sizeof(float), p);
    if (rc || p.trace == nullptr) return rc;
    return wino4_trace_report(ctx, p.trace, nblocks, items, a.cred);
}
// SSDSEG_W4_TRACE: synchronous, prints to stderr
int wino4_trace_report(ssdseg_ctx* ctx, unsigned long long* trace, int nblocks, long long items, int cred) {
    std::vector<unsigned long long> h((size_t)nblocks * 64 * 4);
    SSDSEG_HIP(hipStreamSynchronize(ctx->stream));
    SSDSEG_HIP(hipMemcpy(h.data(), trace, h.size() * 8, hipMemcpyDeviceToHost));
    SSDSEG_HIP(hipFree(trace));
    const int per = (int)((items + nblocks - 1) / nblocks) < 64 ? (int)((items + nblocks - 1) / nblocks) : 64;
    for (int b : {0, 1, nblocks / 2, nblocks - 1}) {
        double loop = 0, epi = 0;
        for (int k = 0; k < per; ++k) {
            loop += (double)(h[((size_t)b * 64 + k) * 4 + 1] - h[((size_t)b * 64 + k) * 4 + 0]);
            epi += (double)(h[((size_t)b * 64 + k) * 4 + 2] - h[((size_t)b * 64 + k) * 4 + 1]);
        }
        const double gap = per > 1 ? ((double)(h[((size_t)b * 64 + per - 1) * 4 + 0] - h[((size_t)b * 64) * 4 + 0]) - (loop - (double)(h[((size_t)b * 64 + per - 1) * 4 + 1] - h[((size_t)b * 64 + per - 1) * 4 + 0])) ) / (per - 1) : 0;
        fprintf(stderr, "w4 trace block %3d: %d items, loop %.0f clk/item (%.0f per 16-channel step), loop end -> item end %.0f, loop end -> next loop start %.0f\n", b, per,
                loop / per, loop / per / (cred / 16), epi / per, gap);
    }
    return 0;
}

int conv3_tiled_launch(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv3TArgs& a, const float* w, int cin, int cout, int mode) {
    switch (p.family) {
        case C3_WINO4: return conv3_wino4_launch(ctx, p, a, w, cin, cout, mode);
        case C3_WINO: return conv3_wino_launch(ctx, p, a, w, cin, cout, mode);
        default: return conv3_tile_launch(ctx, p, a, w, cin, cout, mode);
    }
}

// ---- implicit GEMM
int conv3_gemm_fwd_launch(ssdseg_ctx* ctx, const Conv3Call& c) {
    ssdseg_rowa_args a{};
    a.a0 = c.in->x; a.cs = c.in->scale; a.ct = c.in->shift; a.act = c.in->act; a.lda = c.ldx;
    a.b = c.wgt; a.ldb = c.cout;
    a.out = c.out; a.ldo = c.cout;
    a.stats = c.stats;
    a.I = c.n * c.h * c.w; a.R = 9 * c.cin; a.J = c.cout;
    a.convH = c.h; a.convW = c.w; a.convC = c.cin; a.convSign = 1;
    return ssdseg_rowA_conv3_fwd(ctx, a);
}
int conv3_gemm_bwd_data_launch(ssdseg_ctx* ctx, const Conv3Call& c) {
    ssdseg_rowa_args a{};
    a.a0 = c.dy->g; a.a1 = c.dy->y; a.cs = c.dy->scale; a.ct = c.dy->shift; a.ck1 = c.dy->k1; a.ck0 = c.dy->k0; a.act = c.dy->act;
    a.lda = c.cout;
    a.b = c.wgt; a.ldb = c.cout;
    a.out = c.out; a.ldo = c.ldx;
    a.accumulate = c.accumulate;
    a.I = c.n * c.h * c.w; a.R = 9 * c.cout; a.J = c.cin;
    a.convH = c.h; a.convW = c.w; a.convC = c.cout; a.convSign = -1;   // dx(h,w) gathers dy(h-(kh-1), w-(kw-1))
    return ssdseg_rowA_conv3_bwd_data(ctx, a);
}

// ---- weight gradients
// xsaved != nullptr: the zero-bordered activated input already exists (written by ssdseg_conv3x3_fwd_saved), c.in is not read
int conv3_wino_wgrad_launch(ssdseg_ctx* ctx, const Conv3Call& c, const float* dy, const float* xsaved = nullptr) {
    const int n = c.n, h = c.h, w = c.w, cin = c.cin, cout = c.cout;
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
    if (xsaved == nullptr && (rc = conv3_pad_view(ctx, c.in, c.ldx, xp, n, h, w, cin, 0))) return rc;
    if ((rc = conv3_announce_lds<&conv3_wino_wgrad_kernel>(WWG_LDS_BYTES))) return rc;
    // executed MFMA flops: 16/36 of the direct form's 18 m cin cout
    SSDSEG_LAUNCH(ctx, conv3_cost_bytes(m, cin, cout), 8.0 * m * cin * cout, conv3_wino_wgrad_kernel, dim3((unsigned)nblocks), dim3(WWG_THREADS), WWG_LDS_BYTES, a);
    SSDSEG_LAUNCH_CHECK();
    const long long cn = (long long)cin * cout;
    SSDSEG_LAUNCH(ctx, 4.0 * cn * (16.0 * a.slots + 9.0), 0.0, conv3_wino_wgrad_finalize_kernel, dim3((unsigned)((cn + 255) / 256)), dim3(256), 0, (const float*)a.part, c.out,
                  cin, cout, a.npatches, a.full, a.tail, a.span, a.slots);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// the kernels of the two split-K forms, over the plan's grid
int conv3_wgrad_kernel_launch(ssdseg_ctx* ctx, const Conv3Plan& p, const Wg3TArgs& a, double cost_bytes, double cost_flops) {
    if (int rc = conv3_announce_lds<&conv3_wgrad_tile_kernel>(W3T_LDS_BYTES)) return rc;
    SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, conv3_wgrad_tile_kernel, dim3((unsigned)(p.gx * p.splits)), dim3(W3T_THREADS), W3T_LDS_BYTES, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
int conv3_wgrad_kernel_launch(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv9Args& a, double cost_bytes, double cost_flops) {
    const dim3 grid(p.gx, p.gy, (unsigned)p.splits);
    const size_t lds = (size_t)(C9_PX * (32 * (p.nine == 1 ? 1 : 4) + 4) + 3 * C9_XW * C9_XS) * sizeof(float);
    ctx->timing_view_bytes = a.gs != nullptr ? 4.0 * a.n * a.h * a.w * a.N : 0.0;
    if (p.nine == 12) SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, conv3_wgrad12_kernel, grid, dim3(C12_THREADS), lds, a);
    else if (p.nine == 4) SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, (conv3_wgrad9_kernel<4>), grid, dim3(C9_THREADS), lds, a);
    else SSDSEG_LAUNCH(ctx, cost_bytes, cost_flops, (conv3_wgrad9_kernel<1>), grid, dim3(C9_THREADS), lds, a);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
// dw[9][cin][cout] from the `splits` partial slabs: fixed-order column sum (a copy when there is one slab)
int conv3_wgrad_reduce(ssdseg_ctx* ctx, const float* part, long long splits, int cin, int cout, float* dw) {
    if (splits == 1) {
        SSDSEG_HIP(hipMemcpyAsync(dw, part, (size_t)9 * cin * cout * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    return ssdseg_colsum(ctx, part, (int)splits, 9LL * cin * cout, dw);
}
// the shared tail of the two split-K forms: the plan's splits, their partial slabs, the kernel, the reduce
template <typename Args>
int conv3_wgrad_split_launch(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv3Call& c, Args a) {
    a.n = c.n; a.h = c.h; a.w = c.w; a.K = c.cin; a.N = c.cout;
    a.steps = (decltype(a.steps))p.steps;
    a.steps_per_split = (decltype(a.steps_per_split))p.steps_per_split;
    void* ws;
    int rc = ssdseg_partials(ctx, (size_t)p.splits * 9 * c.cin * c.cout * sizeof(float), &ws);
    if (rc) return rc;
    a.part = (float*)ws;
    const double m = (double)c.n * c.h * c.w;
    if ((rc = conv3_wgrad_kernel_launch(ctx, p, a, conv3_cost_bytes(m, c.cin, c.cout), 18.0 * m * c.cin * c.cout))) return rc;
    return conv3_wgrad_reduce(ctx, a.part, p.splits, c.cin, c.cout, c.out);
}
// halo-tile form (conv3_wgrad_tile.h)
int conv3_tile_wgrad_launch(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv3Call& c) {
    Wg3TArgs a{};
    conv3_set_view(&a, c.in, c.ldx);
    a.g = c.dy->g;
    a.ktiles = cdiv(c.cin, W3T_KT); a.ntiles = cdiv(c.cout, W3T_NT);
    a.strips = cdiv(c.w, W3T_COLS);
    a.x_bytes = (unsigned)((((long long)c.n * c.h * c.w - 1) * c.ldx + c.cin) * 4);
    a.g_bytes = (unsigned)((long long)c.n * c.h * c.w * c.cout * 4);
    return conv3_wgrad_split_launch(ctx, p, c, a);
}
// all nine taps in one pass (conv3_wgrad.h)
int conv3_nine_wgrad_launch(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv3Call& c) {
    Conv9Args a{};
    conv3_set_view(&a, c.in, c.ldx);
    conv3_set_gview(&a, c.dy);
    a.wchunks = cdiv(c.w, C9_PX);
    return conv3_wgrad_split_launch(ctx, p, c, a);
}
int conv3_taps_wgrad_launch(ssdseg_ctx* ctx, const Conv3Call& c) {
    for (int tap = 0; tap < 9; ++tap) {
        ssdseg_wgrad_args a{};
        conv3_set_view(&a, c.in, c.ldx);
        conv3_set_gview(&a, c.dy);
        a.ldy = c.cout;
        a.M = c.n * c.h * c.w; a.K = c.cin; a.N = c.cout;
        a.convH = c.h; a.convW = c.w; a.dh = tap / 3 - 1; a.dw = tap % 3 - 1;
        int rc = ssdseg_wgrad_run(ctx, a, c.out + (size_t)tap * c.cin * c.cout);
        if (rc) return rc;
    }
    return 0;
}

// the table is sized for the largest candidate (ssdseg_conv3x3_parts): zero the rows the planned kernel does not write
int conv3_zero_unwritten_stats(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv3Call& c) {
    if (c.stats == nullptr) return 0;
    const int nparts = conv3_fwd_table_rows(c.n, c.h, c.w, c.cin, c.cout);
    if (nparts > p.rows) SSDSEG_HIP(hipMemsetAsync(c.stats + (size_t)p.rows * 2 * c.cout, 0, (size_t)(nparts - p.rows) * 2 * c.cout * sizeof(float), ctx->stream));
    return 0;
}

// input gradient, with the BatchNorm sums of the layer's input where c.bn != nullptr
int conv3_bwd_data_run(ssdseg_ctx* ctx, const Conv3Plan& p, const Conv3Call& c) {
    const Conv3BnOut* b = c.bn;
    int rc;
    switch (p.family) {
        case C3_NARROW_DIRECT: return ssdseg_conv3n_bwd_bn_direct(ctx, c.in, c.dy, c.wgt, c.out, c.ldx, c.n, c.h, c.w, b->mean, b->invstd, b->dgamma, b->dbeta, b->k1, b->k0);
        case C3_NARROW: return conv3n_bwd_data_launch(ctx, c);      // (the sums ride in its GEMM's epilogue)
        case C3_GEMM: rc = conv3_gemm_bwd_data_launch(ctx, c); break;
        default:
            rc = conv3_tiled_launch(ctx, p, conv3t_args(c.dy->g, nullptr, nullptr, SSDSEG_ACT_NONE, c.cout, c.out, c.ldx, c.accumulate, nullptr, c.n, c.h, c.w, c.cout, c.cin), c.wgt,
                                    c.cin, c.cout, 1);
    }
    if (rc || b == nullptr) return rc;
    return ssdseg_bn_bwd_reduce(ctx, c.out, c.ldx, c.in->x, c.ldx, c.n * c.h * c.w, c.cin, c.in->scale, c.in->shift, b->mean, b->invstd, c.in->act, b->dgamma, b->dbeta, b->k1, b->k0);
}

}  // namespace

extern "C" {

int ssdseg_transpose_w(ssdseg_ctx* ctx, const float* w, float* wt, int cin, int cout, int taps) {
    SSDSEG_LAUNCH(ctx, 8.0 * taps * cin * cout, 0.0, conv3_transpose_w_kernel, dim3(cdiv(cout, 32), cdiv(cin, 32), taps), dim3(256), 0, w, wt, cin, cout);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ dense 3x3 (K6)
int ssdseg_conv3x3_parts(int n, int h, int w, int cin, int cout, int* nparts_host) {
    SSDSEG_ARG(n > 0 && h > 0 && w > 0, 1);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 4);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 5);
    SSDSEG_ARG(nparts_host != nullptr, 6);
    // sized for whichever forward kernel may run: the dispatch switches (SSDSEG_CONV3_*) are read again at launch time
    *nparts_host = conv3_fwd_table_rows(n, h, w, cin, cout);
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
    const Conv3Plan p = conv3_fwd_plan(conv3_switches(), n, h, wdt, ldx, cin, cout);
    const Conv3Call c{n, h, wdt, cin, cout, in, ldx, nullptr, w, y, stats, 0, nullptr};
    int rc = conv3_zero_unwritten_stats(ctx, p, c);
    if (rc) return rc;
    switch (p.family) {
        case C3_NARROW: return conv3n_fwd_launch(ctx, p, c);
        case C3_GEMM: return conv3_gemm_fwd_launch(ctx, c);
        default:
            return conv3_tiled_launch(ctx, p, conv3t_args(in->x, in->scale, in->shift, in->act, ldx, y, cout, 0, stats, n, h, wdt, cin, cout), w, cin, cout, 0);
    }
}

// ---- forward that SAVES its activated input for the weight gradient (large Winograd layers; include/ssdseg.h)
int ssdseg_conv3x3_saved_floats(int n, int h, int w, int cin, int cout, long long* floats_host) {
    SSDSEG_ARG(n > 0 && h > 0 && w > 0, 1);
    SSDSEG_ARG(cin > 0 && cin % 4 == 0, 4);
    SSDSEG_ARG(cout > 0 && cout % 4 == 0, 5);
    SSDSEG_ARG(floats_host != nullptr, 6);
    *floats_host = conv3_saved_pair(conv3_switches(), n, h, w, cin, cout) ? (long long)n * (h + 2) * (w + 2) * cin : 0;
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
    SSDSEG_ARG(need > 0, 6);     // only for shapes ssdseg_conv3x3_saved_floats reports a size for: the plan below is a Winograd one
    // the kernel streams the saved copy, which is dense: row stride cin, whatever ldx is
    const Conv3Plan p = conv3_fwd_plan(conv3_switches(), n, h, wdt, cin, cin, cout);
    const Conv3Call c{n, h, wdt, cin, cout, in, ldx, nullptr, w, y, stats, 0, nullptr};
    rc = conv3_zero_unwritten_stats(ctx, p, c);
    if (rc) return rc;
    if ((rc = conv3_pad_view(ctx, in, ldx, xsaved, n, h, wdt, cin, c_from))) return rc;
    // (the input: pixel (1, 1) of image 0 of the zero-bordered copy)
    Conv3TArgs t = conv3t_args(xsaved + ((long long)(wdt + 2) + 1) * cin, nullptr, nullptr, SSDSEG_ACT_NONE, cin, y, cout, 0, stats, n, h, wdt, cin, cout);
    t.in_hp = h + 2; t.in_wp = wdt + 2;
    return conv3_tiled_launch(ctx, p, t, w, cin, cout, 0);
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
    const Conv3Call c{n, h, wdt, cin, cout, nullptr, cin, nullptr, nullptr, dw, nullptr, 0, nullptr};
    return conv3_wino_wgrad_launch(ctx, c, dy, xsaved);
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
    const Conv3BnOut bn{in_mean, in_invstd, in_dgamma, in_dbeta, in_k1, in_k0};
    const Conv3Call c{n, h, wdt, cin, cout, in, ldx, dy, w, dx, nullptr, 0, &bn};
    return conv3_bwd_data_run(ctx, conv3_bwd_data_plan(conv3_switches(), n, h, wdt, ldx, cin, cout, dy->scale != nullptr, true), c);
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
    const Conv3Call c{n, h, wdt, cin, cout, nullptr, ldx, dy, w, dx, nullptr, accumulate, nullptr};
    return conv3_bwd_data_run(ctx, conv3_bwd_data_plan(conv3_switches(), n, h, wdt, ldx, cin, cout, dy->scale != nullptr, false), c);
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
    const Conv3Plan p = conv3_wgrad_plan(conv3_switches(), ctx->num_cus, n, h, wdt, ldx, cin, cout, dy->scale != nullptr);
    const Conv3Call c{n, h, wdt, cin, cout, in, ldx, dy, nullptr, dw, nullptr, 0, nullptr};
    switch (p.family) {
        case C3W_NARROW: return conv3n_wgrad_launch(ctx, c);
        case C3W_WINO: return conv3_wino_wgrad_launch(ctx, c, dy->g);
        case C3W_TILE: return conv3_tile_wgrad_launch(ctx, p, c);
        case C3W_NINE: return conv3_nine_wgrad_launch(ctx, p, c);
        default: return conv3_taps_wgrad_launch(ctx, c);
    }
}

}  // extern "C"
