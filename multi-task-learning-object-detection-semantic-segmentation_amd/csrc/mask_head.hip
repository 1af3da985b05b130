// Mask head tail of the DeepLabV3+ head, 4 classes, fused: bilinear up-sampling -> Softmax -> weighted cross-entropy or dice
// (reference blocks.py:128-130 + losses.py:175-303), forward and backward, and the soft-Jaccard metric of the same masks
// (metrics.py:35-47), which shares the up-sampling, the softmax and the per-image sums.  Not in the reference: the bootstrapped
// cross-entropy (hard-pixel mining), which keeps the `keep` largest per-pixel cross-entropy terms of every image.
#include "lerp_softmax.h"
#include "radix_select.h"

namespace {

__device__ __forceinline__ float4 up_logits(const float* __restrict__ logits, long long img, int h, int w, int oy, int ox, float ify, float ifx) {
    const Lerp ly = lerp_of(oy, h, ify), lx = lerp_of(ox, w, ifx);
    const float* base = logits + img * h * w * 4;
    const float4 v00 = ld4(base + ((long long)ly.i0 * w + lx.i0) * 4), v01 = ld4(base + ((long long)ly.i0 * w + lx.i1) * 4);
    const float4 v10 = ld4(base + ((long long)ly.i1 * w + lx.i0) * 4), v11 = ld4(base + ((long long)ly.i1 * w + lx.i1) * 4);
    return lerp_blend4(v00, v01, v10, v11, lx.f, ly.f);
}
__device__ __forceinline__ float clip_log(float p) { return logf(fminf(fmaxf(p, KEPS), 1.f - KEPS)); }
__device__ __forceinline__ float inside(float p) { return (p >= KEPS && p <= 1.f - KEPS) ? 1.f : 0.f; }
// sum_c w_c y_c clip_log(p_c) of one pixel, the expression mask_head_fwd_kernel subtracts: negated, the bootstrapped loss's key
__device__ __forceinline__ float ce_term(float4 cw, float4 y, float4 pr) {
    return cw.x * y.x * clip_log(pr.x) + cw.y * y.y * clip_log(pr.y) + cw.z * y.z * clip_log(pr.z) + cw.w * y.w * clip_log(pr.w);
}

// dL/dp of one pixel.  mode 0: weighted cross-entropy, -w_c y_c / clip(p_c) inside the clip interval, 0 outside (App. B.6);
// mode 1 / 2: dice / dice_square (reference losses.py:204-216, 250-262): with the per-image sums I_c = sum y p, T_c = sum (y + p)
// [sum (y^2 + p^2)],  dL/dp_c = A_c y_c + B_c [2 p_c],  A_c = -2 w_c / (T_c + eps),  B_c = w_c (2 I_c + eps) / (T_c + eps)^2
// (cA, cB: written per image by mask_dice_final_kernel);  mode 3: bootstrapped cross-entropy, mode 0's expression (mask_dz selects
// the kept pixels).
constexpr int MASK_BOOTSTRAP = 3;
__device__ __forceinline__ float4 mask_dp(int mode, float4 cw, float4 y, float4 pr, float4 cA, float4 cB) {
    float4 dp;
    if (mode == 0 || mode == MASK_BOOTSTRAP) {
        dp.x = -cw.x * y.x / fminf(fmaxf(pr.x, KEPS), 1.f - KEPS) * inside(pr.x);
        dp.y = -cw.y * y.y / fminf(fmaxf(pr.y, KEPS), 1.f - KEPS) * inside(pr.y);
        dp.z = -cw.z * y.z / fminf(fmaxf(pr.z, KEPS), 1.f - KEPS) * inside(pr.z);
        dp.w = -cw.w * y.w / fminf(fmaxf(pr.w, KEPS), 1.f - KEPS) * inside(pr.w);
    } else {
        const float4 t = mode == 2 ? make_float4(2.f * pr.x, 2.f * pr.y, 2.f * pr.z, 2.f * pr.w) : f4(1.f);
        dp.x = fmaf(cA.x, y.x, cB.x * t.x);
        dp.y = fmaf(cA.y, y.y, cB.y * t.y);
        dp.z = fmaf(cA.z, y.z, cB.z * t.z);
        dp.w = fmaf(cA.w, y.w, cB.w * t.w);
    }
    return dp;
}

// A pixel is labelled iff any component of its one-hot row is non-zero; an all-zero row (a class index >= 4 on the data side, the
// fill_class = 255 padding of crop / mosaic) is void.  The VOID instantiations below leave a void pixel out of T_c, of the kept
// pixels and of the gradient; I_c and the cross-entropy term of a zero row are zero as they stand.
// (An integer test of the bits, the sign shifted out: behind floating-point compares of y the compiler stops contracting y + p in
// mask_iou_partial_kernel as it does in the plain instantiation, and the bit identity without void pixels is lost.)
__device__ __forceinline__ bool labelled(float4 y) {
    return ((__float_as_uint(y.x) | __float_as_uint(y.y) | __float_as_uint(y.z) | __float_as_uint(y.w)) << 1) != 0u;
}

// dz = softmax'(dL/dp) of the full-resolution pixel (oy, ox) of image img, whose one-hot row is y_pixel: up-sampled logits, softmax,
// one-hot read, dL/dp.  Bootstrapped mode: l_pixel is the pixel's loss as the forward STORED it and thr its image's threshold; the
// keep decision is the forward's comparison on the forward's bits (a recomputed loss would be at the mercy of contraction), and a
// dropped pixel's dL/dp is selected to an exact zero row, so its dz is +0.  VOID (the dice modes; a void pixel of the bootstrapped
// loss is dropped by its stored sentinel): a void pixel's dL/dp is that zero row too.
template <bool VOID>
__device__ __forceinline__ float4 mask_dz(const float* logits, long long img, int h, int w, int oy, int ox, float ify, float ifx,
                                          const float* y_pixel, int mode, float4 cw, float4 cA, float4 cB, const float* l_pixel, float thr) {
    const float4 pr = softmax4(up_logits(logits, img, h, w, oy, ox, ify, ifx));
    const float4 y = ld4(y_pixel);
    float4 dp = mask_dp(mode, cw, y, pr, cA, cB);
    const bool kept = (mode != MASK_BOOTSTRAP || *l_pixel >= thr) && (!VOID || labelled(y));
    dp = kept ? dp : f4(0.f);
    const float dot = dp.x * pr.x + dp.y * pr.y + dp.z * pr.z + dp.w * pr.w;
    return make_float4(pr.x * (dp.x - dot), pr.y * (dp.y - dot), pr.z * (dp.z - dot), pr.w * (dp.w - dot));
}

// one pixel's terms of the eight per-image sums of the dice losses and of the soft Jaccard: s[c] = I_c = sum y_c p_c,
// s[4 + c] = T_c = sum (y_c + p_c)  [squared: sum (y_c^2 + p_c^2)]
__device__ __forceinline__ void overlap_sums_add(float (&s)[8], float4 y, float4 pr, bool squared) {
    s[0] = fmaf(y.x, pr.x, s[0]); s[1] = fmaf(y.y, pr.y, s[1]); s[2] = fmaf(y.z, pr.z, s[2]); s[3] = fmaf(y.w, pr.w, s[3]);
    if (squared) {
        s[4] += fmaf(y.x, y.x, pr.x * pr.x); s[5] += fmaf(y.y, y.y, pr.y * pr.y); s[6] += fmaf(y.z, y.z, pr.z * pr.z); s[7] += fmaf(y.w, y.w, pr.w * pr.w);
    } else {
        s[4] += y.x + pr.x; s[5] += y.y + pr.y; s[6] += y.z + pr.z; s[7] += y.w + pr.w;
    }
}
// the same for the VOID kernels: a void pixel leaves T_c as it is.  The new sums are formed by the function above and SELECTED, so
// that the arithmetic (and what the compiler contracts of it) is the plain kernels' and a batch without void pixels gives their
// bits; the I terms of an all-zero y row are zero as they stand.
__device__ __forceinline__ void overlap_sums_add_labelled(float (&s)[8], float4 y, float4 pr, bool squared) {
    float t[8] = {s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
    overlap_sums_add(t, y, pr, squared);
    const bool lab = labelled(y);
#pragma unroll
    for (int k = 0; k < 4; ++k) { s[k] = t[k]; s[4 + k] = lab ? t[4 + k] : s[4 + k]; }
}

// ------------------------------------------------------------------------------------------------ forward
// grid (blocks_per_image, n); partial[n][blocks_per_image] per-image loss partials
__global__ void __launch_bounds__(256) mask_head_fwd_kernel(const float* __restrict__ logits, int h, int w, int fy, int fx,
                                                            const float* __restrict__ y_true, float4 cw, float* __restrict__ prob,
                                                            float* __restrict__ partial) {
    __shared__ float red[1][256];
    const int ho = h * fy, wo = w * fx;
    const long long npix = (long long)ho * wo;
    const long long img = blockIdx.y;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    float loss = 0.f;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(p % wo), oy = (int)(p / wo);
        const float4 pr = softmax4(up_logits(logits, img, h, w, oy, ox, ify, ifx));
        const long long off = (img * npix + p) * 4;
        if (prob) st4(prob + off, pr);
        if (y_true) {
            const float4 y = ld4(y_true + off);
            loss -= cw.x * y.x * clip_log(pr.x) + cw.y * y.y * clip_log(pr.y) + cw.z * y.z * clip_log(pr.z) + cw.w * y.w * clip_log(pr.w);
        }
    }
    if (partial) {
        const float v[1] = {loss};
        block_sum256(v, red);
        if (threadIdx.x == 0) partial[img * gridDim.x + blockIdx.x] = red[0][0];
    }
}

__global__ void mask_loss_final_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ loss, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += (double)partial[(long long)i * nblk + b];
    loss[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------ bootstrapped cross-entropy
// Hard-pixel mining: per image, loss = sum of the pixel losses l_i = -ce_term >= the keep-th largest of them (thresh); every pixel
// tied with that value is kept (no tie-break: the kept count may exceed keep).  The forward stores l (4 B per pixel); an exact
// radix select over its keys (radix_select.h: four 8-bit passes, block-local LDS histograms merged with integer atomics, one
// histogram state per image) finds thresh; the sum pass and the backward kernels compare the stored l with it.

// forward variant: l per pixel instead of the per-block sums (0 - x: an all-zero-weight pixel gives +0, never -0, so that the
// comparison on floats and the order of the keys agree); grid (blocks_per_image, n), the pixel walk of mask_head_fwd_kernel
__global__ void __launch_bounds__(256) mask_head_fwd_pixel_kernel(const float* __restrict__ logits, int h, int w, int fy, int fx,
                                                                  const float* __restrict__ y_true, float4 cw, float* __restrict__ prob,
                                                                  float* __restrict__ pixel_loss) {
    const int ho = h * fy, wo = w * fx;
    const long long npix = (long long)ho * wo;
    const long long img = blockIdx.y;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(p % wo), oy = (int)(p / wo);
        const float4 pr = softmax4(up_logits(logits, img, h, w, oy, ox, ify, ifx));
        const long long off = (img * npix + p) * 4;
        if (prob) st4(prob + off, pr);
        pixel_loss[img * npix + p] = 0.f - ce_term(cw, ld4(y_true + off), pr);
    }
}

// the same l from given probabilities (the standalone loss callable): y_true, p [total][4]
__global__ void __launch_bounds__(256) pixel_ce_kernel(const float* __restrict__ y_true, const float* __restrict__ p, long long total, float4 cw,
                                                       float* __restrict__ pixel_loss) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        pixel_loss[i] = 0.f - ce_term(cw, ld4(y_true + i * 4), ld4(p + i * 4));
}

// Void variants of the two kernels above, grid (blocks_per_image, n): a void pixel stores the sentinel -1 (every labelled l is
// >= +0, so void never outranks it and `l >= thresh` drops it in the sum pass and in the backward as it drops any other pixel),
// and the block's count of labelled pixels goes to labelled_part[n][blocks_per_image], from which bootstrap_keep_kernel forms keep.
constexpr float VOID_LOSS = -1.f;
// (the count is kept per WAVE: every trip adds the population of the wave's ballot, so lane 0, which makes every trip its wave
// makes, holds the wave's count at the end, and the block's is the sum of four numbers: no tree over 256 threads)
__device__ __forceinline__ int labelled_in_wave(bool lab) { return __popcll(__ballot(lab)); }
__device__ __forceinline__ void labelled_count_store(int wave_cnt, int* __restrict__ labelled_part) {
    __shared__ int redc[4];
    if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    if (threadIdx.x == 0) labelled_part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = redc[0] + redc[1] + redc[2] + redc[3];
}
__global__ void __launch_bounds__(256) mask_head_fwd_pixel_void_kernel(const float* __restrict__ logits, int h, int w, int fy, int fx,
                                                                       const float* __restrict__ y_true, float4 cw, float* __restrict__ prob,
                                                                       float* __restrict__ pixel_loss, int* __restrict__ labelled_part) {
    const int ho = h * fy, wo = w * fx;
    const long long npix = (long long)ho * wo;
    const long long img = blockIdx.y;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    int cnt = 0;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(p % wo), oy = (int)(p / wo);
        const float4 pr = softmax4(up_logits(logits, img, h, w, oy, ox, ify, ifx));
        const long long off = (img * npix + p) * 4;
        if (prob) st4(prob + off, pr);
        const float4 y = ld4(y_true + off);
        const bool lab = labelled(y);
        pixel_loss[img * npix + p] = lab ? 0.f - ce_term(cw, y, pr) : VOID_LOSS;
        cnt += labelled_in_wave(lab);
    }
    labelled_count_store(cnt, labelled_part);
}
__global__ void __launch_bounds__(256) pixel_ce_void_kernel(const float* __restrict__ y_true, const float* __restrict__ p, int hw, float4 cw,
                                                            float* __restrict__ pixel_loss, int* __restrict__ labelled_part) {
    const long long base = (long long)blockIdx.y * hw;
    int cnt = 0;
    for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < hw; i += gridDim.x * 256) {
        const float4 y = ld4(y_true + (base + i) * 4);
        const bool lab = labelled(y);
        pixel_loss[base + i] = lab ? 0.f - ce_term(cw, y, ld4(p + (base + i) * 4)) : VOID_LOSS;
        cnt += labelled_in_wave(lab);
    }
    labelled_count_store(cnt, labelled_part);
}
// keep[img] = min(L, max(1, ceil(keep_fraction L))) in double, L = the image's labelled pixels (0 for L = 0): losses.bootstrap_keep
// on the batch the device sees
__global__ void bootstrap_keep_kernel(const int* __restrict__ labelled_part, int nblk, int n, double keep_fraction, int* __restrict__ keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int l = 0;
    for (int b = 0; b < nblk; ++b) l += labelled_part[(long long)i * nblk + b];
    const double want = ceil(keep_fraction * (double)l);
    const int k = want < 1.0 ? 1 : (want > (double)l ? l : (int)want);
    keep[i] = k < l ? k : l;
}

// f(l) for every one of the npix losses of an image, block `blk` of `nblk`: 16-byte reads where the image's row is 16-byte aligned
template <typename F>
__device__ __forceinline__ void for_each_loss(const float* __restrict__ v, int npix, int blk, int nblk, F f) {
    if ((npix & 3) == 0) {
        const int n4 = npix >> 2;
        for (int i = blk * 256 + (int)threadIdx.x; i < n4; i += nblk * 256) {
            const float4 q = ld4(v + 4 * (long long)i);
            f(q.x); f(q.y); f(q.z); f(q.w);
        }
    } else {
        for (int i = blk * 256 + (int)threadIdx.x; i < npix; i += nblk * 256) f(v[i]);
    }
}

// one 8-bit pass of the select, grid (blocks, n): hist [n][4][256], zeroed by the host.  keep_img (void variant, else NULL): k per
// image from device memory; k = 0 (no labelled pixel) selects nothing.  The void variant's sentinels (l < 0) stay out of the
// histogram: k never exceeds the labelled pixels, which all rank above them, and one bin shared by every void pixel of a zoom-out
// would serialise the LDS atomics of the first pass
__global__ void __launch_bounds__(256) bootstrap_hist_kernel(const float* __restrict__ pixel_loss, int npix, int keep,
                                                             const int* __restrict__ keep_img, int* __restrict__ hist, int pass) {
    __shared__ int lh[256];
    __shared__ int bins[256];
    __shared__ unsigned s_prefix;
    __shared__ int s_krem;
    const int t = threadIdx.x;
    int* st = hist + (long long)blockIdx.y * 1024;
    if (keep_img != nullptr) keep = keep_img[blockIdx.y];
    radix_select_prefix(reinterpret_cast<const int(*)[256]>(st), pass, keep, lh, &s_prefix, &s_krem);
    const unsigned prefix = s_prefix;
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    const bool skip_void = keep_img != nullptr;
    bins[t] = 0;
    __syncthreads();
    for_each_loss(pixel_loss + (long long)blockIdx.y * npix, npix, blockIdx.x, gridDim.x, [&](float l) {
        const unsigned key = order_key(l);
        if ((key & himask) == prefix && !(skip_void && l < 0.f)) atomicAdd(&bins[(key >> shift) & 255u], 1);
    });
    __syncthreads();
    if (bins[t] != 0) atomicAdd(&st[pass * 256 + t], bins[t]);
}

// sum pass, grid (blocks, n): thresh[img] = the float of the selected key (+inf where keep_img says k = 0: nothing is kept); per
// block the sum and the count of the kept losses
__global__ void __launch_bounds__(256) bootstrap_sum_kernel(const float* __restrict__ pixel_loss, int npix, int keep,
                                                            const int* __restrict__ keep_img, const int* __restrict__ hist,
                                                            float* __restrict__ thresh, float* __restrict__ partial, int* __restrict__ pcount) {
    __shared__ int lh[256];
    __shared__ float red[1][256];
    __shared__ int redc[1][256];
    __shared__ unsigned s_prefix;
    __shared__ int s_krem;
    if (keep_img != nullptr) keep = keep_img[blockIdx.y];
    radix_select_prefix(reinterpret_cast<const int(*)[256]>(hist + (long long)blockIdx.y * 1024), 4, keep, lh, &s_prefix, &s_krem);
    const float thr = keep == 0 ? INFINITY : order_key_value(s_prefix);
    if (blockIdx.x == 0 && threadIdx.x == 0) thresh[blockIdx.y] = thr;
    float sum = 0.f;
    int cnt = 0;
    for_each_loss(pixel_loss + (long long)blockIdx.y * npix, npix, blockIdx.x, gridDim.x, [&](float l) {
        const bool kept = l >= thr;
        sum += kept ? l : 0.f;
        cnt += kept ? 1 : 0;
    });
    const float v[1] = {sum};
    const int c[1] = {cnt};
    block_sum256(v, red);
    block_sum256(c, redc);
    if (threadIdx.x == 0) {
        partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = red[0][0];
        pcount[(long long)blockIdx.y * gridDim.x + blockIdx.x] = redc[0][0];
    }
}

__global__ void bootstrap_final_kernel(const float* __restrict__ partial, const int* __restrict__ pcount, int nblk, int n, float* __restrict__ loss,
                                       int* __restrict__ kept) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    int c = 0;
    for (int b = 0; b < nblk; ++b) {
        s += (double)partial[(long long)i * nblk + b];
        c += pcount[(long long)i * nblk + b];
    }
    if (loss != nullptr) loss[i] = (float)s;
    if (kept != nullptr) kept[i] = c;
}

// dice / dice_square forward: probabilities (optional) and per-block partial sums (I_c, T_c); grid (blocks_per_image, n),
// partial[n][blocks_per_image][8].  VOID: a void pixel adds nothing to T_c (overlap_sums_add)
template <bool VOID>
__global__ void __launch_bounds__(256) mask_head_fwd_dice_kernel(const float* __restrict__ logits, int h, int w, int fy, int fx,
                                                                 const float* __restrict__ y_true, int squared, float* __restrict__ prob,
                                                                 float* __restrict__ partial) {
    __shared__ float red[8][256];
    const int ho = h * fy, wo = w * fx;
    const long long npix = (long long)ho * wo;
    const long long img = blockIdx.y;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(p % wo), oy = (int)(p / wo);
        const float4 pr = softmax4(up_logits(logits, img, h, w, oy, ox, ify, ifx));
        const long long off = (img * npix + p) * 4;
        if (prob) st4(prob + off, pr);
        const float4 y = ld4(y_true + off);
        if constexpr (VOID) overlap_sums_add_labelled(s, y, pr, squared);
        else overlap_sums_add(s, y, pr, squared);
    }
    block_sum256(s, red);
    const int t = threadIdx.x;
    if (t < 8) partial[(img * gridDim.x + blockIdx.x) * 8 + t] = red[t][0];
}

// per image: I_c, T_c (partials summed in index order, double), the loss, and the backward coefficients coef[img] = (A_0..3, B_0..3)
__global__ void mask_dice_final_kernel(const float* __restrict__ partial, int nblk, int n, float4 cw, float* __restrict__ loss,
                                       float* __restrict__ coef) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nblk; ++b)
#pragma unroll
        for (int v = 0; v < 8; ++v) s[v] += (double)partial[((long long)i * nblk + b) * 8 + v];
    const double w[4] = {cw.x, cw.y, cw.z, cw.w};
    const double eps = (double)KEPS;
    double l = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double den = s[4 + c] + eps, num = 2.0 * s[c] + eps;
        l += w[c] * (1.0 - num / den);
        if (coef != nullptr) {
            coef[i * 8 + c] = (float)(-2.0 * w[c] / den);
            coef[i * 8 + 4 + c] = (float)(w[c] * num / (den * den));
        }
    }
    if (loss != nullptr) loss[i] = (float)l;
}

// ------------------------------------------------------------------------------------------------ backward
// dlogits(low res) = sum over the full-res pixels that interpolate from it of weight * dz, dz = softmax'(dL/dp)
template <bool VOID>
__global__ void __launch_bounds__(256) mask_head_bwd_kernel(const float* __restrict__ logits, int n, int h, int w, int fy, int fx,
                                                            const float* __restrict__ y_true, float4 cw, float loss_scale,
                                                            float* __restrict__ dlogits, int mode, const float* __restrict__ coef,
                                                            const float* __restrict__ pixel_loss, const float* __restrict__ thresh) {
    const int ho = h * fy, wo = w * fx;
    const long long total = (long long)n * h * w;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ix = (int)(i % w);
        const int iy = (int)((i / w) % h);
        const long long img = i / ((long long)w * h);
        const LerpWindow win = lerp_window(iy, ix, h, w, fy, fx);
        float4 acc = f4(0.f);
        const bool dice = mode == 1 || mode == 2;
        const float4 cA = dice ? ld4(coef + img * 8) : f4(0.f), cB = dice ? ld4(coef + img * 8 + 4) : f4(0.f);
        const float thr = mode == MASK_BOOTSTRAP ? thresh[img] : 0.f;
        for (int oy = win.oy0; oy <= win.oy1; ++oy) {
            const float wy = lerp_weight(oy, iy, h, ify);
            if (wy == 0.f) continue;
            for (int ox = win.ox0; ox <= win.ox1; ++ox) {
                const float wx = lerp_weight(ox, ix, w, ifx);
                if (wx == 0.f) continue;
                const long long pix = (img * ho + oy) * wo + ox;
                axpy4(acc, wy * wx * loss_scale,
                      mask_dz<VOID>(logits, img, h, w, oy, ox, ify, ifx, y_true + pix * 4, mode, cw, cA, cB, pixel_loss ? pixel_loss + pix : nullptr, thr));
            }
        }
        st4(dlogits + i * 4, acc);
    }
}

// The tile kernels below form the same sum with each full-resolution pixel's dz computed ONCE per block instead of once per
// contributing low-resolution pixel (x16 up-sampling area: every dz has up to four takers, and the kernel above re-does the bilinear
// gather, the softmax and the one-hot read for each of them: 0.31 ms at 480x640, batch 32).  A block owns a TL x TL tile of
// low-resolution pixels and first writes the dz of the R x R full-resolution pixels that can reach them into LDS, R = TL*F + F:
// low-res pixel i takes weight from [i*F - F/2, i*F + F + F/2 - 1] (lerp_window), so a tile of TL pixels draws from TL*F + F
// indices, starting at i0*F - F/2.  This is that phase, for a block of NT threads; it ends with the barrier.
struct MaskTile {
    long long img;
    int iy0, ix0;      // first low-resolution pixel of the tile
    int oyb, oxb;      // full-resolution pixel of dz[0]
};
template <int F, int TL, int NT, bool VOID>
__device__ __forceinline__ MaskTile mask_dz_fill(float4* dz, const float* logits, int h, int w, const float* y_true, float4 cw, int mode,
                                                 const float* coef, const float* pixel_loss, const float* thresh) {
    constexpr int R = TL * F + F;
    const int ho = h * F, wo = w * F;
    const float inv = 1.f / (float)F;
    const int tiles_x = (w + TL - 1) / TL, tiles_y = (h + TL - 1) / TL;
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y;
    MaskTile t;
    t.img = b / tiles_y;
    t.iy0 = ty * TL; t.ix0 = tx * TL;
    t.oyb = t.iy0 * F - F / 2; t.oxb = t.ix0 * F - F / 2;
    const bool dice = mode == 1 || mode == 2;
    const float4 cA = dice ? ld4(coef + t.img * 8) : f4(0.f), cB = dice ? ld4(coef + t.img * 8 + 4) : f4(0.f);
    const float thr = mode == MASK_BOOTSTRAP ? thresh[t.img] : 0.f;
    for (int i = threadIdx.x; i < R * R; i += NT) {
        const int ry = i / R, rx = i - ry * R;
        const int oy = t.oyb + ry, ox = t.oxb + rx;
        float4 v = f4(0.f);
        if (oy >= 0 && oy < ho && ox >= 0 && ox < wo) {
            const long long pix = (t.img * ho + oy) * wo + ox;
            v = mask_dz<VOID>(logits, t.img, h, w, oy, ox, inv, inv, y_true + pix * 4, mode, cw, cA, cB, pixel_loss ? pixel_loss + pix : nullptr, thr);
        }
        dz[i] = v;
    }
    __syncthreads();
    return t;
}

// x4: after the dz phase every thread gathers the window of its low-resolution pixel from LDS.  Each dz is the same expression and
// the window is walked in the same (oy, ox) order as in mask_head_bwd_kernel: results are bit-identical.
template <int F, int TL, bool VOID>
__global__ void __launch_bounds__(TL * TL) mask_head_bwd_tile_kernel(const float* __restrict__ logits, int n, int h, int w,
                                                                       const float* __restrict__ y_true, float4 cw, float loss_scale,
                                                                       float* __restrict__ dlogits, int mode, const float* __restrict__ coef,
                                                                       const float* __restrict__ pixel_loss, const float* __restrict__ thresh) {
    constexpr int R = TL * F + F;
    extern __shared__ float4 dz[];                    // [R][R]
    const MaskTile tile = mask_dz_fill<F, TL, TL * TL, VOID>(dz, logits, h, w, y_true, cw, mode, coef, pixel_loss, thresh);
    const float inv = 1.f / (float)F;
    const int ly = threadIdx.x / TL, lx = threadIdx.x - ly * TL;
    const int iy = tile.iy0 + ly, ix = tile.ix0 + lx;
    if (iy >= h || ix >= w) return;
    const LerpWindow win = lerp_window(iy, ix, h, w, F, F);
    // the column weights of the window once per thread, not once per (row, column) -- the same lerp_weight values, the same products and
    // the same summation order (rows, then columns, zero weights skipped): bit-identical, ~130 weight evaluations per thread less
    constexpr int WMAX = lerp_window_max(F);
    float wxs[WMAX];
#pragma unroll
    for (int k = 0; k < WMAX; ++k) wxs[k] = (win.ox0 + k <= win.ox1) ? lerp_weight(win.ox0 + k, ix, w, inv) : 0.f;
    float4 acc = f4(0.f);
    for (int oy = win.oy0; oy <= win.oy1; ++oy) {
        const float wy = lerp_weight(oy, iy, h, inv);
        if (wy == 0.f) continue;
        const float4* drow = dz + (oy - tile.oyb) * R + (win.ox0 - tile.oxb);
#pragma unroll
        for (int k = 0; k < WMAX; ++k) {
            const float wx = wxs[k];
            if (wx == 0.f) continue;
            axpy4(acc, wy * wx * loss_scale, drow[k]);
        }
    }
    st4(dlogits + ((tile.img * h + iy) * w + ix) * 4, acc);
}

// Larger factors (x8: ShuffleNetV2's 60 x 80 logits): a window holds (2F + F/2)^2 full-resolution pixels, so the gather is split over
// PARTS threads per low-resolution pixel (interleaved rows, partials folded in part order: deterministic, but not the summation
// order of the one-thread kernel) and all TL^2 * PARTS threads share the dz phase.
template <int F, int TL, int PARTS, bool VOID>
__global__ void __launch_bounds__(TL * TL * PARTS) mask_head_bwd_tile_split_kernel(const float* __restrict__ logits, int n, int h, int w,
                                                                                     const float* __restrict__ y_true, float4 cw, float loss_scale,
                                                                                     float* __restrict__ dlogits, int mode, const float* __restrict__ coef,
                                                                                     const float* __restrict__ pixel_loss,
                                                                                     const float* __restrict__ thresh) {
    constexpr int R = TL * F + F;
    extern __shared__ float4 dz[];                    // [R][R] + [PARTS][TL * TL]
    float4* red = dz + R * R;
    const MaskTile tile = mask_dz_fill<F, TL, TL * TL * PARTS, VOID>(dz, logits, h, w, y_true, cw, mode, coef, pixel_loss, thresh);
    const float inv = 1.f / (float)F;
    const int pix = threadIdx.x % (TL * TL), part = threadIdx.x / (TL * TL);
    const int ly = pix / TL, lx = pix - ly * TL;
    const int iy = tile.iy0 + ly, ix = tile.ix0 + lx;
    const bool live = iy < h && ix < w;
    const LerpWindow win = lerp_window(iy, ix, h, w, F, F);      // (in front of the branch: measured 2 % faster than inside it)
    float4 acc = f4(0.f);
    if (live) {
        for (int oy = win.oy0 + part; oy <= win.oy1; oy += PARTS) {
            const float wy = lerp_weight(oy, iy, h, inv);
            if (wy == 0.f) continue;
            for (int ox = win.ox0; ox <= win.ox1; ++ox) {
                const float wx = lerp_weight(ox, ix, w, inv);
                if (wx == 0.f) continue;
                axpy4(acc, wy * wx * loss_scale, dz[(oy - tile.oyb) * R + (ox - tile.oxb)]);
            }
        }
    }
    red[part * TL * TL + pix] = acc;
    __syncthreads();
    if (part == 0 && live) {
        float4 s = red[pix];
#pragma unroll
        for (int q = 1; q < PARTS; ++q) add4(s, red[q * TL * TL + pix]);
        st4(dlogits + ((tile.img * h + iy) * w + ix) * 4, s);
    }
}

// ------------------------------------------------------------------------------------------------ soft Jaccard metric
// (reference metrics.py:35-47; per-image values, Keras averages them): per image and class  inter = sum t*p,  total = sum (t + p)
// over the full-resolution pixels; p = softmax(upsampled logits) when FROM_LOGITS (the training path never stores the
// probabilities) or the given probabilities.  Two-level reduction in fixed order.  grid (nblk, n) -> partial[n][nblk][8]
// VOID: total over the labelled pixels only (as in mask_head_fwd_dice_kernel)
template <bool FROM_LOGITS, bool VOID>
__global__ void __launch_bounds__(256) mask_iou_partial_kernel(const float* __restrict__ src, int h, int w, int fy, int fx,
                                                               const float* __restrict__ y_true, float* __restrict__ partial) {
    __shared__ float red[1][256];
    const int ho = h * fy, wo = w * fx;
    const long long npix = (long long)ho * wo;
    const int img = blockIdx.y;
    const float ify = 1.f / (float)fy, ifx = 1.f / (float)fx;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const int oy = (int)(i / wo), ox = (int)(i - (long long)oy * wo);
        float4 pr;
        if (FROM_LOGITS) pr = softmax4(up_logits(src, img, h, w, oy, ox, ify, ifx));
        else pr = ld4(src + ((long long)img * npix + i) * 4);
        const float4 y = ld4(y_true + ((long long)img * npix + i) * 4);
        if constexpr (VOID) overlap_sums_add_labelled(acc, y, pr, false);
        else overlap_sums_add(acc, y, pr, false);
    }
    for (int k = 0; k < 8; ++k) {       // one value per pass: 1 KiB of LDS
        __syncthreads();
        const float v[1] = {acc[k]};
        block_sum256(v, red);
        if (threadIdx.x == 0) partial[((long long)img * gridDim.x + blockIdx.x) * 8 + k] = red[0][0];
    }
}
__global__ void mask_iou_finish_kernel(const float* __restrict__ partial, int nblk, int n, float4 cw, float* __restrict__ out) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= n) return;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < nblk; ++q)
        for (int k = 0; k < 8; ++k) s[k] += partial[((long long)img * nblk + q) * 8 + k];
    const float w[4] = {cw.x, cw.y, cw.z, cw.w};
    float m = 0.f;
    for (int c = 0; c < 4; ++c) m += s[c] / (s[4 + c] - s[c] + KEPS) * w[c];   // metrics.py:41-45
    out[img] = m;
}

// ------------------------------------------------------------------------------------------------ host
// blocks per image of a two-level sum over npix full-resolution pixels: eight pixels per thread, at most `cap`
int partial_blocks(long long npix, int cap) {
    const long long nblk = (npix + 256 * 8 - 1) / (256 * 8);
    return (int)(nblk > cap ? cap : (nblk < 1 ? 1 : nblk));
}

// launches Kernel with `lds` bytes of dynamic LDS, more than the default limit: raised on the kernel's first launch (one flag per
// kernel: Kernel is a template argument).  `name`: what the launch leaves in the timing registry.
template <auto Kernel, typename... Args>
int launch_with_lds(ssdseg_ctx* ctx, const char* name, double bytes, long long blocks, int threads, size_t lds, Args... args) {
    static bool configured = false;
    if (!configured) {
        SSDSEG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        configured = true;
    }
    SSDSEG_LAUNCH_NAMED(ctx, name, bytes, 0.0, Kernel, dim3((unsigned)blocks), dim3(threads), lds, args...);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// mode 0: cross-entropy (cwh: the class weights); 1 / 2: dice / dice_square (coef: mask_dice_final_kernel's); MASK_BOOTSTRAP:
// bootstrapped cross-entropy (cwh, and the forward's pixel_loss [n][H*W] and thresh [n]; both NULL in every other mode).  VOID: the
// instantiations that give a void pixel a zero gradient row (the dice modes of the _void entries), under names of their own
template <bool VOID = false>
int mask_head_bwd_launch(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int fy, int fx, const float* y_true, const float* cwh,
                         float loss_scale, float* dlogits, int mode, const float* coef, const float* pixel_loss = nullptr,
                         const float* thresh = nullptr) {
    const double bytes = (pixel_loss ? 20.0 : 16.0) * n * h * fy * wdt * fx;
    const float4 cw = f4_of(cwh);
    const bool tiles = env_pick("SSDSEG_MASK_BWD", {"gather"}) == 0;      // "gather": the one-thread-per-pixel kernel (A/B runs, parity tests)
    if (tiles && fy == 4 && fx == 4) {
        constexpr int F = 4, TL = 16, R = TL * F + F;
        return launch_with_lds<mask_head_bwd_tile_kernel<F, TL, VOID>>(ctx, VOID ? "(mask_head_bwd_tile_kernel<F, TL, VOID>)" : "(mask_head_bwd_tile_kernel<F, TL>)", bytes, (long long)n * cdiv(h, TL) * cdiv(wdt, TL),
                                                                  TL * TL, R * R * sizeof(float4), logits, n, h, wdt, y_true, cw, loss_scale, dlogits, mode, coef,
                                                                  pixel_loss, thresh);
    }
    if (tiles && fy == 8 && fx == 8) {
        constexpr int F = 8, TL = 8, PARTS = 4, R = TL * F + F;
        return launch_with_lds<mask_head_bwd_tile_split_kernel<F, TL, PARTS, VOID>>(
            ctx, VOID ? "(mask_head_bwd_tile_split_kernel<F, TL, PARTS, VOID>)" : "(mask_head_bwd_tile_split_kernel<F, TL, PARTS>)", bytes,
                                                                               (long long)n * cdiv(h, TL) * cdiv(wdt, TL), TL * TL * PARTS,
                                                                               (size_t)(R * R + PARTS * TL * TL) * sizeof(float4), logits, n, h, wdt, y_true, cw,
                                                                               loss_scale, dlogits, mode, coef, pixel_loss, thresh);
    }
    SSDSEG_LAUNCH_NAMED(ctx, VOID ? "mask_head_bwd_kernel<VOID>" : "mask_head_bwd_kernel", bytes, 0.0, mask_head_bwd_kernel<VOID>,
                        dim3(ew_blocks((long long)n * h * wdt)), dim3(256), 0, logits, n, h, wdt, fy, fx, y_true, cw, loss_scale, dlogits, mode, coef,
                        pixel_loss, thresh);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

// The select and the sum over pixel_loss [n][npix]: thresh [n], and loss / kept [n] where asked for.  Workspace (behind `front`
// bytes the caller keeps): hist [n][4][256] | partial [n][nblk] | pcount [n][nblk].
int bootstrap_blocks(int npix) {
    const int nblk = cdiv(npix, 256 * 16);
    return nblk > 32 ? 32 : nblk;
}
size_t bootstrap_ws_bytes(int n, int npix) { return (size_t)n * (4096 + 8 * (size_t)bootstrap_blocks(npix)); }
// keep_img (void variant, else NULL): k per image from device memory in place of `keep`.
int bootstrap_select_launch(ssdseg_ctx* ctx, const float* pixel_loss, int n, int npix, int keep, const int* keep_img, void* ws, float* thresh,
                            int* kept, float* loss) {
    const int nblk = bootstrap_blocks(npix);
    int* hist = (int*)ws;
    float* partial = (float*)((char*)ws + (size_t)n * 4096);
    int* pcount = (int*)(partial + (size_t)n * nblk);
    SSDSEG_HIP(hipMemsetAsync(hist, 0, (size_t)n * 4096, ctx->stream));
    for (int pass = 0; pass < 4; ++pass) {
        SSDSEG_LAUNCH(ctx, 4.0 * n * npix, 0.0, bootstrap_hist_kernel, dim3(nblk, n), dim3(256), 0, pixel_loss, npix, keep, keep_img, hist, pass);
        SSDSEG_LAUNCH_CHECK();
    }
    SSDSEG_LAUNCH(ctx, 4.0 * n * npix, 0.0, bootstrap_sum_kernel, dim3(nblk, n), dim3(256), 0, pixel_loss, npix, keep, keep_img, (const int*)hist, thresh,
                  partial, pcount);
    SSDSEG_LAUNCH_CHECK();
    if (loss != nullptr || kept != nullptr) {
        SSDSEG_LAUNCH(ctx, 8.0 * n * nblk, 0.0, bootstrap_final_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (const float*)partial, (const int*)pcount, nblk,
                      n, loss, kept);
        SSDSEG_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

// what the mask-head entry points check first (a macro: SSDSEG_ARG reports under, and returns from, the entry point's own name)
#define MASK_HEAD_ARGS()                                                                                       \
    SSDSEG_ARG(ctx != nullptr, 1);                                                                             \
    SSDSEG_ARG(logits != nullptr, 2);                                                                          \
    SSDSEG_ARG(n > 0 && h > 0 && wdt > 0, 3);                                                                  \
    SSDSEG_ARG(c == 4, 6);   /* the reference itself hard-codes depth 4 (layers.py:204, models.py:250-253) */  \
    SSDSEG_ARG(fy >= 1 && fx >= 1, 7)

#define MASK_DICE_FWD_ARGS()                                                                          \
    MASK_HEAD_ARGS();                                                                                 \
    SSDSEG_ARG(n <= 65535, 3);   /* the image is gridDim.y of mask_head_fwd_dice_kernel */            \
    SSDSEG_ARG(y_true != nullptr, 9);                                                                 \
    SSDSEG_ARG(class_weights_host != nullptr, 10);                                                    \
    SSDSEG_ARG(loss != nullptr || coef != nullptr, 13)
#define MASK_DICE_BWD_ARGS()             \
    MASK_HEAD_ARGS();                    \
    SSDSEG_ARG(y_true != nullptr, 9);    \
    SSDSEG_ARG(coef != nullptr, 10);     \
    SSDSEG_ARG(dlogits != nullptr, 13)

#define MASK_IOU_ARGS()                                                                                                       \
    SSDSEG_ARG(ctx != nullptr, 1);                                                                                            \
    SSDSEG_ARG(src != nullptr, 2);                                                                                            \
    SSDSEG_ARG(n > 0 && n <= 65535 && h > 0 && wdt > 0, 3);   /* the image is gridDim.y of mask_iou_partial_kernel */         \
    SSDSEG_ARG(c == 4, 6);                                                                                                    \
    SSDSEG_ARG(fy >= 1 && fx >= 1 && (from_logits || (fy == 1 && fx == 1)), 7);                                               \
    SSDSEG_ARG(y_true != nullptr, 10);                                                                                        \
    SSDSEG_ARG(class_weights_host != nullptr, 11);                                                                            \
    SSDSEG_ARG(out != nullptr, 12)

namespace {
template <bool VOID>
int mask_iou_launch(ssdseg_ctx* ctx, const float* src, int n, int h, int wdt, int fy, int fx, int from_logits, const float* y_true,
                    const float* class_weights_host, float* out) {
    const long long npix = (long long)h * fy * wdt * fx;
    const int nblk = partial_blocks(npix, 64);
    void* ws;
    int rc = ssdseg_workspace(ctx, (size_t)n * nblk * 8 * sizeof(float), &ws);
    if (rc) return rc;
    const double bytes = 16.0 * n * npix * (from_logits ? 1.0 : 2.0);
    if (from_logits)
        SSDSEG_LAUNCH_NAMED(ctx, VOID ? "mask_iou_partial_kernel<true, VOID>" : "mask_iou_partial_kernel<true>", bytes, 0.0,
                            (mask_iou_partial_kernel<true, VOID>), dim3(nblk, n), dim3(256), 0, src, h, wdt, fy, fx, y_true, (float*)ws);
    else
        SSDSEG_LAUNCH_NAMED(ctx, VOID ? "mask_iou_partial_kernel<false, VOID>" : "mask_iou_partial_kernel<false>", bytes, 0.0,
                            (mask_iou_partial_kernel<false, VOID>), dim3(nblk, n), dim3(256), 0, src, h, wdt, fy, fx, y_true, (float*)ws);
    SSDSEG_LAUNCH_CHECK();
    SSDSEG_LAUNCH(ctx, 0.0, 0.0, mask_iou_finish_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (const float*)ws, nblk, n, f4_of(class_weights_host), out);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

template <bool VOID>
int mask_dice_fwd_launch(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int fy, int fx, const float* y_true,
                                const float* class_weights_host, int squared, float* prob, float* loss, float* coef) {
    const long long npix = (long long)h * fy * wdt * fx;
    const int nblk = partial_blocks(npix, 256);
    void* ws;
    int rc = ssdseg_workspace(ctx, (size_t)n * nblk * 8 * sizeof(float), &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH_NAMED(ctx, VOID ? "mask_head_fwd_dice_kernel<VOID>" : "mask_head_fwd_dice_kernel", 16.0 * n * npix * (1 + (prob ? 1 : 0)), 0.0,
                        mask_head_fwd_dice_kernel<VOID>, dim3(nblk, n), dim3(256), 0, logits, h, wdt, fy, fx, y_true, squared ? 1 : 0, prob, (float*)ws);
    SSDSEG_LAUNCH_CHECK();
    SSDSEG_LAUNCH(ctx, 32.0 * n * nblk, 0.0, mask_dice_final_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (const float*)ws, nblk, n,
                  f4_of(class_weights_host), loss, coef);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

int ssdseg_mask_head_fwd(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                         const float* class_weights_host, float* prob, float* loss) {
    MASK_HEAD_ARGS();
    SSDSEG_ARG(n <= 65535, 3);   // the image is gridDim.y of mask_head_fwd_kernel
    SSDSEG_ARG((loss == nullptr) || (y_true != nullptr && class_weights_host != nullptr), 9);
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    const long long npix = (long long)h * fy * wdt * fx;
    const int nblk = partial_blocks(npix, 256);
    float* partial = nullptr;
    if (loss) {
        void* ws;
        int rc = ssdseg_workspace(ctx, (size_t)n * nblk * sizeof(float), &ws);
        if (rc) return rc;
        partial = (float*)ws;
    }
    SSDSEG_LAUNCH(ctx, 16.0 * n * npix * ((y_true ? 1 : 0) + (prob ? 1 : 0)), 0.0, mask_head_fwd_kernel, dim3(nblk, n), dim3(256), 0, logits, h,
                  wdt, fy, fx, loss ? y_true : nullptr, f4_of(loss ? class_weights_host : zero), prob, partial);
    SSDSEG_LAUNCH_CHECK();
    if (loss) {
        SSDSEG_LAUNCH(ctx, 4.0 * n * nblk, 0.0, mask_loss_final_kernel, dim3(cdiv(n, 64)), dim3(64), 0, partial, nblk, loss, n);
        SSDSEG_LAUNCH_CHECK();
    }
    return 0;
}

int ssdseg_mask_head_fwd_dice(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                              const float* class_weights_host, int squared, float* prob, float* loss, float* coef) {
    MASK_DICE_FWD_ARGS();
    return mask_dice_fwd_launch<false>(ctx, logits, n, h, wdt, fy, fx, y_true, class_weights_host, squared, prob, loss, coef);
}

int ssdseg_mask_head_fwd_dice_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                                   const float* class_weights_host, int squared, float* prob, float* loss, float* coef) {
    MASK_DICE_FWD_ARGS();
    return mask_dice_fwd_launch<true>(ctx, logits, n, h, wdt, fy, fx, y_true, class_weights_host, squared, prob, loss, coef);
}

int ssdseg_mask_head_bwd_dice(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                              const float* coef, int squared, float loss_scale, float* dlogits) {
    MASK_DICE_BWD_ARGS();
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    return mask_head_bwd_launch(ctx, logits, n, h, wdt, fy, fx, y_true, zero, loss_scale, dlogits, squared ? 2 : 1, coef);
}

int ssdseg_mask_head_bwd_dice_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                                   const float* coef, int squared, float loss_scale, float* dlogits) {
    MASK_DICE_BWD_ARGS();
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    return mask_head_bwd_launch<true>(ctx, logits, n, h, wdt, fy, fx, y_true, zero, loss_scale, dlogits, squared ? 2 : 1, coef);
}

int ssdseg_mask_head_bwd(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                         const float* class_weights_host, float loss_scale, float* dlogits) {
    MASK_HEAD_ARGS();
    SSDSEG_ARG(y_true != nullptr, 9);
    SSDSEG_ARG(class_weights_host != nullptr, 10);
    SSDSEG_ARG(dlogits != nullptr, 12);
    return mask_head_bwd_launch(ctx, logits, n, h, wdt, fy, fx, y_true, class_weights_host, loss_scale, dlogits, 0, nullptr);
}

int ssdseg_mask_head_fwd_bootstrap(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                                   const float* class_weights_host, int keep, float* prob, float* pixel_loss, float* thresh, int* kept,
                                   float* loss) {
    MASK_HEAD_ARGS();
    SSDSEG_ARG(n <= 65535, 3);   // the image is gridDim.y of mask_head_fwd_pixel_kernel and of the select's kernels
    SSDSEG_ARG(y_true != nullptr, 9);
    SSDSEG_ARG(class_weights_host != nullptr, 10);
    const long long npix = (long long)h * fy * wdt * fx;
    SSDSEG_ARG(npix <= 0x7FFFFFFFLL, 4);
    SSDSEG_ARG(keep >= 1 && keep <= npix, 11);
    SSDSEG_ARG(pixel_loss != nullptr, 13);
    SSDSEG_ARG(thresh != nullptr, 14);
    void* ws;
    int rc = ssdseg_workspace(ctx, bootstrap_ws_bytes(n, (int)npix), &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, n * npix * (20.0 + (prob ? 16.0 : 0.0)), 0.0, mask_head_fwd_pixel_kernel, dim3(partial_blocks(npix, 256), n), dim3(256), 0, logits,
                  h, wdt, fy, fx, y_true, f4_of(class_weights_host), prob, pixel_loss);
    SSDSEG_LAUNCH_CHECK();
    return bootstrap_select_launch(ctx, pixel_loss, n, (int)npix, keep, nullptr, ws, thresh, kept, loss);
}

int ssdseg_mask_head_bwd_bootstrap(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                                   const float* class_weights_host, const float* pixel_loss, const float* thresh, float loss_scale,
                                   float* dlogits) {
    MASK_HEAD_ARGS();
    SSDSEG_ARG(y_true != nullptr, 9);
    SSDSEG_ARG(class_weights_host != nullptr, 10);
    SSDSEG_ARG(pixel_loss != nullptr, 11);
    SSDSEG_ARG(thresh != nullptr, 12);
    SSDSEG_ARG(dlogits != nullptr, 14);
    return mask_head_bwd_launch(ctx, logits, n, h, wdt, fy, fx, y_true, class_weights_host, loss_scale, dlogits, MASK_BOOTSTRAP, nullptr, pixel_loss,
                                thresh);
}

int ssdseg_bootstrap_ce_loss(ssdseg_ctx* ctx, const float* y_true, const float* p, int n, int hw, int c, const float* class_weights_host,
                             int keep, float* loss) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(y_true != nullptr, 2);
    SSDSEG_ARG(p != nullptr, 3);
    SSDSEG_ARG(n > 0 && hw > 0, 4);
    SSDSEG_ARG(c == 4, 6);
    SSDSEG_ARG(class_weights_host != nullptr, 7);
    SSDSEG_ARG(keep >= 1 && keep <= hw, 8);
    SSDSEG_ARG(loss != nullptr, 9);
    // workspace: pixel_loss [n][hw] | thresh [n] (both rounded up to 16 bytes) | the select's
    const size_t pl_bytes = ((size_t)n * hw * 4 + 15) & ~(size_t)15, th_bytes = ((size_t)n * 4 + 15) & ~(size_t)15;
    void* ws;
    int rc = ssdseg_workspace(ctx, pl_bytes + th_bytes + bootstrap_ws_bytes(n, hw), &ws);
    if (rc) return rc;
    float* pixel_loss = (float*)ws;
    float* thresh = (float*)((char*)ws + pl_bytes);
    const long long total = (long long)n * hw;
    SSDSEG_LAUNCH(ctx, 36.0 * total, 0.0, pixel_ce_kernel, dim3(ew_blocks(total)), dim3(256), 0, y_true, p, total, f4_of(class_weights_host), pixel_loss);
    SSDSEG_LAUNCH_CHECK();
    return bootstrap_select_launch(ctx, pixel_loss, n, hw, keep, nullptr, (char*)ws + pl_bytes + th_bytes, thresh, nullptr, loss);
}

int ssdseg_mask_head_fwd_bootstrap_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                                        const float* class_weights_host, double keep_fraction, float* prob, float* pixel_loss, float* thresh,
                                        int* keep, int* kept, float* loss) {
    MASK_HEAD_ARGS();
    SSDSEG_ARG(n <= 65535, 3);   // the image is gridDim.y of mask_head_fwd_pixel_void_kernel and of the select's kernels
    SSDSEG_ARG(y_true != nullptr, 9);
    SSDSEG_ARG(class_weights_host != nullptr, 10);
    const long long npix = (long long)h * fy * wdt * fx;
    SSDSEG_ARG(npix <= 0x7FFFFFFFLL, 4);
    SSDSEG_ARG(keep_fraction > 0.0 && keep_fraction <= 1.0, 11);
    SSDSEG_ARG(pixel_loss != nullptr, 13);
    SSDSEG_ARG(thresh != nullptr, 14);
    SSDSEG_ARG(keep != nullptr, 15);
    // workspace: labelled_part [n][nblk] (rounded up to 16 bytes) | the select's
    const int nblk = partial_blocks(npix, 256);
    const size_t lp_bytes = ((size_t)n * nblk * 4 + 15) & ~(size_t)15;
    void* ws;
    int rc = ssdseg_workspace(ctx, lp_bytes + bootstrap_ws_bytes(n, (int)npix), &ws);
    if (rc) return rc;
    SSDSEG_LAUNCH(ctx, n * npix * (20.0 + (prob ? 16.0 : 0.0)), 0.0, mask_head_fwd_pixel_void_kernel, dim3(nblk, n), dim3(256), 0, logits, h, wdt, fy, fx,
                  y_true, f4_of(class_weights_host), prob, pixel_loss, (int*)ws);
    SSDSEG_LAUNCH_CHECK();
    SSDSEG_LAUNCH(ctx, 4.0 * n * nblk, 0.0, bootstrap_keep_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (const int*)ws, nblk, n, keep_fraction, keep);
    SSDSEG_LAUNCH_CHECK();
    return bootstrap_select_launch(ctx, pixel_loss, n, (int)npix, 0, keep, (char*)ws + lp_bytes, thresh, kept, loss);
}

// (a void pixel's stored loss is below every thresh: the plain backward's comparison drops it)
int ssdseg_mask_head_bwd_bootstrap_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx, const float* y_true,
                                        const float* class_weights_host, const float* pixel_loss, const float* thresh, float loss_scale,
                                        float* dlogits) {
    MASK_HEAD_ARGS();
    SSDSEG_ARG(y_true != nullptr, 9);
    SSDSEG_ARG(class_weights_host != nullptr, 10);
    SSDSEG_ARG(pixel_loss != nullptr, 11);
    SSDSEG_ARG(thresh != nullptr, 12);
    SSDSEG_ARG(dlogits != nullptr, 14);
    return mask_head_bwd_launch(ctx, logits, n, h, wdt, fy, fx, y_true, class_weights_host, loss_scale, dlogits, MASK_BOOTSTRAP, nullptr, pixel_loss,
                                thresh);
}

int ssdseg_bootstrap_ce_loss_void(ssdseg_ctx* ctx, const float* y_true, const float* p, int n, int hw, int c, const float* class_weights_host,
                                  double keep_fraction, float* loss) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(y_true != nullptr, 2);
    SSDSEG_ARG(p != nullptr, 3);
    SSDSEG_ARG(n > 0 && n <= 65535 && hw > 0 && hw < (1 << 30), 4);   // the image is gridDim.y of pixel_ce_void_kernel; its pixel index is an int
    SSDSEG_ARG(c == 4, 6);
    SSDSEG_ARG(class_weights_host != nullptr, 7);
    SSDSEG_ARG(keep_fraction > 0.0 && keep_fraction <= 1.0, 8);
    SSDSEG_ARG(loss != nullptr, 9);
    // workspace: pixel_loss [n][hw] | thresh [n] | keep [n] | labelled_part [n][nblk] (each rounded up to 16 bytes) | the select's
    const int nblk = partial_blocks(hw, 256);
    const size_t pl_bytes = ((size_t)n * hw * 4 + 15) & ~(size_t)15, th_bytes = ((size_t)n * 4 + 15) & ~(size_t)15,
                 lp_bytes = ((size_t)n * nblk * 4 + 15) & ~(size_t)15;
    void* ws;
    int rc = ssdseg_workspace(ctx, pl_bytes + 2 * th_bytes + lp_bytes + bootstrap_ws_bytes(n, hw), &ws);
    if (rc) return rc;
    float* pixel_loss = (float*)ws;
    float* thresh = (float*)((char*)ws + pl_bytes);
    int* keep = (int*)((char*)ws + pl_bytes + th_bytes);
    int* labelled_part = (int*)((char*)ws + pl_bytes + 2 * th_bytes);
    SSDSEG_LAUNCH(ctx, 36.0 * n * hw, 0.0, pixel_ce_void_kernel, dim3(nblk, n), dim3(256), 0, y_true, p, hw, f4_of(class_weights_host), pixel_loss,
                  labelled_part);
    SSDSEG_LAUNCH_CHECK();
    SSDSEG_LAUNCH(ctx, 4.0 * n * nblk, 0.0, bootstrap_keep_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (const int*)labelled_part, nblk, n, keep_fraction, keep);
    SSDSEG_LAUNCH_CHECK();
    return bootstrap_select_launch(ctx, pixel_loss, n, hw, 0, keep, (char*)ws + pl_bytes + 2 * th_bytes + lp_bytes, thresh, nullptr, loss);
}

int ssdseg_metric_mask_iou(ssdseg_ctx* ctx, const float* src, int n, int h, int wdt, int c, int fy, int fx, int from_logits,
                           const float* y_true, const float* class_weights_host, float* out) {
    MASK_IOU_ARGS();
    return mask_iou_launch<false>(ctx, src, n, h, wdt, fy, fx, from_logits, y_true, class_weights_host, out);
}

int ssdseg_metric_mask_iou_void(ssdseg_ctx* ctx, const float* src, int n, int h, int wdt, int c, int fy, int fx, int from_logits,
                                const float* y_true, const float* class_weights_host, float* out) {
    MASK_IOU_ARGS();
    return mask_iou_launch<true>(ctx, src, n, h, wdt, fy, fx, from_logits, y_true, class_weights_host, out);
}

}  // extern "C"
