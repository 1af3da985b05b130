// Test-set evaluation on the device (reference NB03#cell21-29): the two reductions that turn the inference engine's outputs into
// the numbers evaluators.py reports, so that neither the (N, H, W, C) probabilities nor anything else of that size goes to the host.
//   ssdseg_eval_mask_jaccard   jaccard_iou_semantic_segmentation (reference evaluators.py:189-247) per image and class, straight
//                              from the `output-mask` probabilities and the uint8 class indices a compact / resident batch holds:
//                              y = (index == class) (an index >= c is an all-zero one-hot pixel, tf.one_hot), I = sum y*p,
//                              T = sum (y + p), iou = I / (T - I + 1e-7).  The one-hot mask is never built: I sums p where the
//                              index names the class, and sum y is an integer count.  Per-block partials in the ctx workspace, then
//                              a finish kernel that adds them in index order in double: the same bits on every run.
//   ssdseg_eval_mask_scores    the same pass with two options: the totals over the labelled pixels only (index < c; ignore_void), and
//                              the hard confusion counts M[true][argmax p] of the labelled pixels per image, from the probabilities the
//                              Jaccard sums already hold in registers -- 16 bytes per pixel are read once.  The counts are wave-wide
//                              ballot populations (integers, one accumulator per cell and wave), folded like the Jaccard sums.
//   ssdseg_eval_det_best_iou   for every row of ssdseg_combined_nms' output the largest IoU with a ground-truth box of the same
//                              label (reference evaluators.py:6-62, the float32 expressions of evaluators._iou_boxes_pred_vs_true in
//                              the same order, no FMA contraction); the host thresholds it for as many AP thresholds as it likes.
#include "common.h"

namespace {

constexpr int EVAL_THREADS = 256, EVAL_WAVES = EVAL_THREADS / 64;
constexpr int EVAL_CMAX = 8;                 // classes, as inputs.hip
constexpr int EVAL_WORDS = 3 * EVAL_CMAX;    // one block's partial: I[8], P[8] (float), count[8] (int32)

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one pixel of class index k with probabilities p[0..C): I += p[k] (when k < C), P += p, count[k] += 1
// VOID: P only where the pixel is labelled (0 <= k < C)
template <int C, bool VOID>
__device__ __forceinline__ void jaccard_pixel(int k, const float* p, float* accI, float* accP, int* accN) {
    const bool lab = !VOID || (unsigned)k < (unsigned)C;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const bool y = k == j;
        accI[j] += y ? p[j] : 0.f;
        accP[j] += lab ? p[j] : 0.f;
        accN[j] += y ? 1 : 0;
    }
}

// the confusion cell of a pixel: true class k (a row only when 0 <= k < c), predicted class = the first largest probability
// (np.argmax); -1 for a pixel without a row
template <int C>
__device__ __forceinline__ int confusion_code(int k, const float* p, int c) {
    int pred = 0;
    float best = p[0];
#pragma unroll
    for (int j = 1; j < C; ++j)
        if (j < c && p[j] > best) { best = p[j]; pred = j; }
    return (unsigned)k < (unsigned)c ? k * c + pred : -1;
}
// cnt[i] += the wave's pixels of cell i.  Called by every lane of the wave (code -1: no pixel); cnt is the same in all of them.
template <int NC>
__device__ __forceinline__ void confusion_count(int code, int ncell, int* cnt) {
#pragma unroll
    for (int i = 0; i < NC; ++i)
        if (i < ncell) cnt[i] += __popcll(__ballot(code == i));
}
// the block's cells -> cpart[ncell]: the waves in index order
template <int NC>
__device__ __forceinline__ void confusion_block_store(const int* cnt, int ncell, int* __restrict__ cpart) {
    __shared__ int redc[EVAL_WAVES][NC];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NC; ++i) redc[wv][i] = cnt[i];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < ncell) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < EVAL_WAVES; ++k) s += redc[k][t];
        cpart[t] = s;
    }
}

// the block's sums -> part[24]: butterfly within each wave, then the waves in index order (a fixed order either way)
// (NA: length of the accumulator arrays; classes j >= c hold nothing and are not stored)
template <int NA>
__device__ __forceinline__ void jaccard_block_store(const float* accI, const float* accP, const int* accN, int c, float* __restrict__ part) {
    __shared__ float redf[EVAL_WAVES][2 * EVAL_CMAX];
    __shared__ int redn[EVAL_WAVES][EVAL_CMAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        if (j < c) {                                          // wave-uniform
            const float si = wave_sum(accI[j]), sp = wave_sum(accP[j]);
            const int sn = wave_sum_i(accN[j]);
            if (lane == 0) { redf[wv][j] = si; redf[wv][EVAL_CMAX + j] = sp; redn[wv][j] = sn; }
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < EVAL_WORDS && (t & (EVAL_CMAX - 1)) < c) {
        if (t < 2 * EVAL_CMAX) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < EVAL_WAVES; ++k) s += redf[k][t];
            part[t] = s;
        } else {
            int s = 0;
#pragma unroll
            for (int k = 0; k < EVAL_WAVES; ++k) s += redn[k][t - 2 * EVAL_CMAX];
            reinterpret_cast<int*>(part)[t] = s;
        }
    }
}

// c == 4, prob 16-byte aligned.  grid (nblk, n); a wave takes 256 consecutive pixels per step: lane l loads the dword of class
// indices of pixels 4l .. 4l + 3 (256 bytes per wave) and, four times, the float4 of pixel 64j + l (1 KiB per wave, consecutive
// lanes on consecutive 16 bytes); the index of that pixel is byte l % 4 of lane 16j + l / 4's dword.  The dwords start at the
// image's first 4-byte-aligned index (`head` pixels in, hw need not be a multiple of 4); the head and the tail past the last whole
// dword -- at most 6 pixels -- go through byte loads in block 0.  CONF: also cpart[n][nblk][16], the block's confusion cells.
template <bool VOID, bool CONF>
__global__ void __launch_bounds__(EVAL_THREADS) jaccard_partial4_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ midx, int hw,
                                                                        float* __restrict__ part, int* __restrict__ cpart) {
    const int img = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint8_t* m = midx + (long long)img * hw;
    const float* p = prob + (long long)img * hw * 4;
    int head = (int)((4u - (unsigned)((uintptr_t)m & 3u)) & 3u);
    if (head > hw) head = hw;
    const int nvec = (hw - head) >> 2;                       // whole dwords of indices
    const int nchunk = (nvec + 63) >> 6;
    const uint32_t* mv = reinterpret_cast<const uint32_t*>(m + head);
    const float* pv = p + (long long)head * 4;
    float accI[4] = {0.f, 0.f, 0.f, 0.f}, accP[4] = {0.f, 0.f, 0.f, 0.f};
    int accN[4] = {0, 0, 0, 0};
    int cnt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = blockIdx.x * EVAL_WAVES + wv; q < nchunk; q += gridDim.x * EVAL_WAVES) {      // wave-uniform trip count
        const int g = q * 64 + lane;
        const uint32_t mine = g < nvec ? mv[g] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t word = (uint32_t)__shfl((int)mine, j * 16 + (lane >> 2), 64);
            const int gj = q * 64 + j * 16 + (lane >> 2);    // the dword this pixel's index sits in
            int code = -1;
            if (gj < nvec) {
                const float4 v = ld4(pv + ((long long)q * 256 + j * 64 + lane) * 4);
                const float pp[4] = {v.x, v.y, v.z, v.w};
                const int k = (int)((word >> (8 * (lane & 3))) & 0xffu);
                jaccard_pixel<4, VOID>(k, pp, accI, accP, accN);
                if constexpr (CONF) code = confusion_code<4>(k, pp, 4);
            }
            if constexpr (CONF) confusion_count<16>(code, 16, cnt);
        }
    }
    if (blockIdx.x == 0) {
        int code = -1;
        if (threadIdx.x < 8) {
            const int t = threadIdx.x;
            const int px = t < 4 ? (t < head ? t : -1) : head + 4 * nvec + (t - 4);
            if (px >= 0 && px < hw) {
                const float pp[4] = {p[(long long)px * 4], p[(long long)px * 4 + 1], p[(long long)px * 4 + 2], p[(long long)px * 4 + 3]};
                jaccard_pixel<4, VOID>((int)m[px], pp, accI, accP, accN);
                if constexpr (CONF) code = confusion_code<4>((int)m[px], pp, 4);
            }
        }
        if constexpr (CONF) confusion_count<16>(code, 16, cnt);
    }
    jaccard_block_store<4>(accI, accP, accN, 4, part + ((long long)img * gridDim.x + blockIdx.x) * EVAL_WORDS);
    if constexpr (CONF) confusion_block_store<16>(cnt, 16, cpart + ((long long)img * gridDim.x + blockIdx.x) * 16);
}

// any c <= 8, any alignment: one pixel per thread and step (every lane of a wave makes the same number of trips: the ballots of
// confusion_count need them all); cpart[n][nblk][c * c]
template <bool VOID, bool CONF>
__global__ void __launch_bounds__(EVAL_THREADS) jaccard_partial_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ midx, int hw, int c,
                                                                       float* __restrict__ part, int* __restrict__ cpart) {
    const int img = blockIdx.y;
    const uint8_t* m = midx + (long long)img * hw;
    const float* p = prob + (long long)img * hw * c;
    float accI[EVAL_CMAX], accP[EVAL_CMAX];
    int accN[EVAL_CMAX];
#pragma unroll
    for (int j = 0; j < EVAL_CMAX; ++j) { accI[j] = 0.f; accP[j] = 0.f; accN[j] = 0; }
    int cnt[CONF ? EVAL_CMAX * EVAL_CMAX : 1];
#pragma unroll
    for (int j = 0; j < (CONF ? EVAL_CMAX * EVAL_CMAX : 1); ++j) cnt[j] = 0;
    for (int i0 = blockIdx.x * EVAL_THREADS; i0 < hw; i0 += gridDim.x * EVAL_THREADS) {      // block-uniform trip count
        const int i = i0 + threadIdx.x;
        int code = -1;
        if (i < hw) {
            const int k = m[i];
            float pp[EVAL_CMAX];
#pragma unroll
            for (int j = 0; j < EVAL_CMAX; ++j) pp[j] = j < c ? p[(long long)i * c + j] : 0.f;
            jaccard_pixel<EVAL_CMAX, VOID>(k < c ? k : -1, pp, accI, accP, accN);
            if constexpr (CONF) code = confusion_code<EVAL_CMAX>(k, pp, c);
        }
        if constexpr (CONF) confusion_count<EVAL_CMAX * EVAL_CMAX>(code, c * c, cnt);
    }
    jaccard_block_store<EVAL_CMAX>(accI, accP, accN, c, part + ((long long)img * gridDim.x + blockIdx.x) * EVAL_WORDS);
    if constexpr (CONF) confusion_block_store<EVAL_CMAX * EVAL_CMAX>(cnt, c * c, cpart + ((long long)img * gridDim.x + blockIdx.x) * c * c);
}

// iou[img][class] from the nblk block partials, added in index order in double (reference evaluators.py:236-241)
__global__ void __launch_bounds__(64) jaccard_finish_kernel(const float* __restrict__ part, int nblk, int n, int c, float* __restrict__ iou) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n * c) return;
    const int img = i / c, k = i - img * c;
    double si = 0.0, sp = 0.0;
    long long sn = 0;
    for (int q = 0; q < nblk; ++q) {
        const float* r = part + ((long long)img * nblk + q) * EVAL_WORDS;
        si += (double)r[k];
        sp += (double)r[EVAL_CMAX + k];
        sn += reinterpret_cast<const int*>(r)[2 * EVAL_CMAX + k];
    }
    const double total = (double)sn + sp;                    // sum (y + p)
    iou[i] = (float)(si / (total - si + 1e-7));
}

// confusion[img][true][pred] and void_pixels[img] = hw - the pixels that name a class, from the block partials (integers; either
// output may be NULL)
__global__ void __launch_bounds__(64) confusion_finish_kernel(const float* __restrict__ part, const int* __restrict__ cpart, int nblk, int n, int c, int hw,
                                                              int* __restrict__ confusion, int* __restrict__ void_pixels) {
    const int i = blockIdx.x * 64 + threadIdx.x, cc = c * c;
    if (confusion != nullptr && i < n * cc) {
        const int img = i / cc, cell = i - img * cc;
        int s = 0;
        for (int q = 0; q < nblk; ++q) s += cpart[((long long)img * nblk + q) * cc + cell];
        confusion[i] = s;
    }
    if (void_pixels != nullptr && i < n) {
        int s = 0;
        for (int q = 0; q < nblk; ++q)
            for (int k = 0; k < c; ++k) s += reinterpret_cast<const int*>(part + ((long long)i * nblk + q) * EVAL_WORDS)[2 * EVAL_CMAX + k];
        void_pixels[i] = hw - s;
    }
}

// one thread per prediction row: evaluators._iou_boxes_pred_vs_true(...).max(axis=1) in float32, operation for operation
__global__ void __launch_bounds__(64) det_best_iou_kernel(const float* __restrict__ det, const float* __restrict__ gt, const int32_t* __restrict__ gt_count,
                                                          int n, int r, int gmax, float* __restrict__ best) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n * r) return;
    const int img = i / r;
    const float* d = det + (long long)i * 6;                 // (label, confidence, x0, y0, x1, y1)
    const float label = d[0], x0 = d[2], y0 = d[3], x1 = d[4], y1 = d[5];
    float b = 0.f;
    int cnt = gt_count[img];
    cnt = cnt < 0 ? 0 : (cnt > gmax ? gmax : cnt);
    if (label != 0.f) {
        const float area_p = (x1 - x0 + 1.f) * (y1 - y0 + 1.f);
        for (int g = 0; g < cnt; ++g) {
            const float* t = gt + ((long long)img * gmax + g) * 5;      // (label, xmin, ymin, xmax, ymax)
            if (t[0] != label) continue;
            const float iw = fmaxf(0.f, fminf(x1, t[3]) - fmaxf(x0, t[1]) + 1.f);
            const float ih = fmaxf(0.f, fminf(y1, t[4]) - fmaxf(y0, t[2]) + 1.f);
            const float inter = iw * ih;
            const float area_t = (t[3] - t[1] + 1.f) * (t[4] - t[2] + 1.f);
            b = fmaxf(b, inter / (area_p + area_t - inter + 1e-7f));
        }
    }
    best[i] = b;
}

// the one pass over the probabilities and its finish kernels; <false, false> is ssdseg_eval_mask_jaccard, under the kernel names it
// has always had in the timing registry
template <bool VOID, bool CONF>
int mask_scores_launch(ssdseg_ctx* ctx, const float* prob, const uint8_t* mask_index_u8, int n, int hw, int c, float* iou_out, int* confusion_out,
                       int* void_out) {
    const bool vec = c == 4 && ((uintptr_t)prob & 15) == 0;
    // enough blocks to fill the chip, no more than ~2048 in all, no more than the image has steps for
    const int steps = vec ? cdiv(hw, 4 * EVAL_THREADS) : cdiv(hw, EVAL_THREADS);
    int nblk = 2048 / n;
    nblk = nblk < 1 ? 1 : (nblk > steps ? steps : nblk);
    const size_t part_bytes = (size_t)n * nblk * EVAL_WORDS * sizeof(float);
    void* ws = nullptr;
    int rc = ssdseg_workspace(ctx, part_bytes + (CONF ? (size_t)n * nblk * c * c * sizeof(int) : 0), &ws);
    if (rc) return rc;
    float* part = static_cast<float*>(ws);
    int* cpart = CONF ? reinterpret_cast<int*>(static_cast<char*>(ws) + part_bytes) : nullptr;
    const double bytes = (double)n * hw * (4.0 * c + 1.0) + 4.0 * (3 * c + (CONF ? c * c : 0)) * n * nblk;
    constexpr bool plain = !VOID && !CONF;
    if (vec)
        SSDSEG_LAUNCH_NAMED(ctx, plain ? "jaccard_partial4_kernel" : (CONF ? (VOID ? "jaccard_partial4_kernel<VOID, CONF>" : "jaccard_partial4_kernel<CONF>")
                                                                            : "jaccard_partial4_kernel<VOID>"),
                            bytes, 3.0 * c * n * hw, (jaccard_partial4_kernel<VOID, CONF>), dim3(nblk, n), dim3(EVAL_THREADS), 0, prob, mask_index_u8, hw,
                            part, cpart);
    else
        SSDSEG_LAUNCH_NAMED(ctx, plain ? "jaccard_partial_kernel" : (CONF ? (VOID ? "jaccard_partial_kernel<VOID, CONF>" : "jaccard_partial_kernel<CONF>")
                                                                           : "jaccard_partial_kernel<VOID>"),
                            bytes, 3.0 * c * n * hw, (jaccard_partial_kernel<VOID, CONF>), dim3(nblk, n), dim3(EVAL_THREADS), 0, prob, mask_index_u8, hw,
                            c, part, cpart);
    SSDSEG_LAUNCH_CHECK();
    if (iou_out != nullptr) {
        SSDSEG_LAUNCH(ctx, 4.0 * 3 * c * n * nblk + 4.0 * n * c, 0.0, jaccard_finish_kernel, dim3(cdiv(n * c, 64)), dim3(64), 0, (const float*)part, nblk,
                      n, c, iou_out);
        SSDSEG_LAUNCH_CHECK();
    }
    if (confusion_out != nullptr || void_out != nullptr) {
        SSDSEG_LAUNCH(ctx, 4.0 * (c * c + c) * n * nblk, 0.0, confusion_finish_kernel, dim3(cdiv(n * c * c, 64)), dim3(64), 0, (const float*)part,
                      (const int*)cpart, nblk, n, c, hw, confusion_out, void_out);
        SSDSEG_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

// what the two mask entries check first
#define EVAL_MASK_ARGS()                                                                                                        \
    SSDSEG_ARG(ctx != nullptr, 1);                                                                                              \
    SSDSEG_ARG(prob != nullptr, 2);                                                                                             \
    SSDSEG_ARG(mask_index_u8 != nullptr, 3);                                                                                    \
    SSDSEG_ARG(n > 0 && n <= 65535, 4);                      /* one grid row per image */                                       \
    SSDSEG_ARG(hw > 0 && hw < (1 << 28), 5);                 /* in-image element offsets and the chunk arithmetic in 32 bits */ \
    SSDSEG_ARG(c >= 1 && c <= EVAL_CMAX, 6)

extern "C" {

int ssdseg_eval_mask_jaccard(ssdseg_ctx* ctx, const float* prob, const uint8_t* mask_index_u8, int n, int hw, int c, float* iou_out) {
    EVAL_MASK_ARGS();
    SSDSEG_ARG(iou_out != nullptr, 7);
    return mask_scores_launch<false, false>(ctx, prob, mask_index_u8, n, hw, c, iou_out, nullptr, nullptr);
}

int ssdseg_eval_mask_scores(ssdseg_ctx* ctx, const float* prob, const uint8_t* mask_index_u8, int n, int hw, int c, int ignore_void, float* iou_out,
                            int32_t* confusion_out, int32_t* void_out) {
    EVAL_MASK_ARGS();
    SSDSEG_ARG(iou_out != nullptr || confusion_out != nullptr || void_out != nullptr, 8);
    const bool conf = confusion_out != nullptr;
    if (ignore_void) {
        return conf ? mask_scores_launch<true, true>(ctx, prob, mask_index_u8, n, hw, c, iou_out, confusion_out, void_out)
                    : mask_scores_launch<true, false>(ctx, prob, mask_index_u8, n, hw, c, iou_out, confusion_out, void_out);
    }
    return conf ? mask_scores_launch<false, true>(ctx, prob, mask_index_u8, n, hw, c, iou_out, confusion_out, void_out)
                : mask_scores_launch<false, false>(ctx, prob, mask_index_u8, n, hw, c, iou_out, confusion_out, void_out);
}

int ssdseg_eval_det_best_iou(ssdseg_ctx* ctx, const float* det, const float* gt, const int32_t* gt_count, int n, int r, int gmax, float* best_out) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(det != nullptr, 2);
    SSDSEG_ARG(gt != nullptr, 3);
    SSDSEG_ARG(gt_count != nullptr, 4);
    SSDSEG_ARG(n > 0, 5);
    SSDSEG_ARG(r > 0 && (long long)n * r < (1LL << 31), 6);
    SSDSEG_ARG(gmax > 0, 7);
    SSDSEG_ARG(best_out != nullptr, 8);
    SSDSEG_LAUNCH(ctx, 28.0 * n * r + 20.0 * n * gmax, 0.0, det_best_iou_kernel, dim3(cdiv((long long)n * r, 64)), dim3(64), 0, det, gt, gt_count, n, r,
                  gmax, best_out);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
