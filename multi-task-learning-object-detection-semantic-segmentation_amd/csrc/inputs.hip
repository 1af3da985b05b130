// Device-side expansion of a COMPACT training batch (the step on the input side of the hot path).
//
// The reference's tf.data map (DataEncoderDecoder.read_and_encode, reference datacoder.py:302-347) produces, per sample, a
// float32 image, a float32 one-hot mask and -- through _encode_ground_truth_labels_boxes (:177-300) -- the encoded anchors;
// with a random horizontal flip applied to all three consistently (:337-345, boxes x -> W - x :202-203, quirk Q8).  Handing those
// float tensors to the GPU costs 285 MB per batch-32 step over PCIe (118 MB images, 157 MB one-hot masks, 10 MB anchors).
// Here the host hands over what the files contain -- uint8 pixels, uint8 class indices, the (label, box) rows -- 39 MB, and
//   ssdseg_expand_inputs   casts the pixels to float32 (tf.cast :327), one-hots the class index (tf.one_hot :332: an index >=
//                          depth gives an all-zero row) and mirrors both left-right where the sample's flip flag is set
//                          (tf.image.flip_left_right :341-342), writing straight into the engine's input / target buffers;
//   ssdseg_flip_gt_boxes   mirrors the ground-truth rows of the flagged samples (xmin' = W - xmax, xmax' = W - xmin :202-203),
// after which ssdseg_encode_targets (boxes.hip) runs on the device as before.  Byte / integer work throughout: results are
// bit-identical to the host path (tests/test_gpu_input_pipeline.py).
// And DataEncoderDecoder.augmentation_rgb_channels (reference datacoder.py:434-466), the colour step the reference maps over every
// batch after read_and_encode, on the same compact pixels:
//   ssdseg_rgb_augment     hue shift, saturation scale (two RGB->HSV->RGB round trips), contrast about the per-(image, channel)
//                          mean, brightness shift and the clip to [0, 255] -- with ONE draw set for the batch -- from the uint8
//                          pixels straight into the engine's float32 input buffer, mirrored where flagged.  Float work: it follows
//                          the host spec datacoder._augment_rgb operation for operation (no FMA contraction, correctly rounded
//                          divisions), so it agrees with it to rounding (tests/test_gpu_rgb_augmentation.py).
// And the reference's tf.data chain itself (NB03#cell8: shuffle(len) -> map(read_and_encode) -> batch -> map(augmentation)) for a
// training set that lives in HBM (datacoder.ResidentDataset): indexed forms of the above that build a batch from pools,
//   ssdseg_gather_inputs   output sample n = pool sample index[n], expanded (or colour-augmented) and mirrored where flagged:
//                          the bits of ssdseg_expand_inputs / ssdseg_rgb_augment on the same samples stacked on the host;
//   ssdseg_gather_gt       its ground-truth rows and count, mirrored as ssdseg_flip_gt_boxes does, rows past the count zero
// (tests/test_gpu_resident_dataset.py).
// Each pass is ONE kernel -- expand_kernel, rgb_stats_kernel, rgb_apply_kernel -- templated on how a block learns its source
// sample and its flip flag (batch_sel.h): plain_sel for the compact entry points, gather_sel for the indexed ones; and one host
// function per pass (expand_pass, rgb_passes) that both kinds of entry point call.  In-image offsets are 32-bit (every entry
// point refuses an image of 2^31 bytes or more), sample offsets 64-bit.
#include <cmath>

#include "batch_sel.h"

namespace {

// the x extent of a box mirrored left-right: xmin' = W - xmax, xmax' = W - xmin (quirk Q8)
__device__ __forceinline__ void mirror_box(float width, float& xmin, float& xmax) {
    const float lo = width - xmax;
    xmax = width - xmin;
    xmin = lo;
}

// in place: rows past the count and unflagged samples are left alone
__global__ void flip_gt_boxes_kernel(float* __restrict__ gt, const int* __restrict__ count, const uint8_t* __restrict__ flip, int b, int gmax,
                                     float width) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // over b * gmax rows
    if (i >= b * gmax) return;
    const int n = i / gmax, g = i - n * gmax;
    if (flip[n] == 0 || g >= count[n]) return;
    float* r = gt + (long long)i * 5;                          // (label, xmin, ymin, xmax, ymax)
    mirror_box(width, r[1], r[3]);
}

// ---------------------------------------------------------------- colour augmentation (datacoder._augment_rgb)
// NumPy's float `x % 1.0` (fmod, then + 1 for a negative remainder; a zero remainder is +0): x - trunc(x) IS fmod(x, 1) exactly
__device__ __forceinline__ float pymod1(float x) {
    float r = x - truncf(x);
    if (r < 0.f) r += 1.f;
    return r == 0.f ? 0.f : r;
}

// datacoder._rgb_to_hsv on one pixel (h in [0, 1], s in [0, 1], v = max)
__device__ __forceinline__ void rgb_to_hsv(float r, float g, float b, float& h, float& s, float& v) {
#pragma clang fp contract(off)
    const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b), d = mx - mn;
    s = mx > 0.f ? d / mx : 0.f;
    const float dd = d > 0.f ? d : 1.f;
    const float hh = mx == r ? (g - b) / dd : (mx == g ? 2.f + (b - r) / dd : 4.f + (r - g) / dd);
    h = d > 0.f ? pymod1(hh / 6.f) : 0.f;
    v = mx;
}

// datacoder._hsv_to_rgb: channel = v - v*s*clip(min(k, 4 - k), 0, 1), k = (n + 6h) mod 6 for n = 5, 3, 1.  n + 6h lies in
// [1, 11], where the mod is one exact subtraction.
__device__ __forceinline__ float hsv_channel(float n, float dh, float s, float v) {
#pragma clang fp contract(off)
    float k = n + dh;
    k = k >= 6.f ? k - 6.f : k;
    const float t = fminf(fmaxf(fminf(k, 4.f - k), 0.f), 1.f);
    return v - v * s * t;
}

// hue shift then saturation scale: the image whose per-channel mean the contrast step centres on
__device__ __forceinline__ void hue_saturation(float& r, float& g, float& b, float hue, float sat) {
#pragma clang fp contract(off)
    float h, s, v;
    rgb_to_hsv(r, g, b, h, s, v);
    h = pymod1(h + hue);
    float dh = h * 6.f;
    r = hsv_channel(5.f, dh, s, v); g = hsv_channel(3.f, dh, s, v); b = hsv_channel(1.f, dh, s, v);
    rgb_to_hsv(r, g, b, h, s, v);
    s = fminf(fmaxf(s * sat, 0.f), 1.f);
    dh = h * 6.f;
    r = hsv_channel(5.f, dh, s, v); g = hsv_channel(3.f, dh, s, v); b = hsv_channel(1.f, dh, s, v);
}

__device__ __forceinline__ float contrast_brightness(float q, float m, float con, float bri) {
#pragma clang fp contract(off)
    return fminf(fmaxf((q - m) * con + m + bri, 0.f), 255.f);
}

constexpr int AUG_THREADS = 256, AUG_PIX = 4;      // 4 pixels per thread: 12 bytes in (3 dwords), 12 floats out (3 x float4)
constexpr int AUG_BLOCK_PIX = AUG_THREADS * AUG_PIX;

// the 12 bytes of pixels [p, p + 4) of one image as 3 dwords (needs p % 4 == 0 and an image of a multiple of 4 pixels)
__device__ __forceinline__ void load4px(const uint8_t* img, int p, float px[12]) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(img + (long long)p * 3);
    const uint32_t a[3] = {q[0], q[1], q[2]};
#pragma unroll
    for (int j = 0; j < 12; ++j) px[j] = (float)((a[j >> 2] >> (8 * (j & 3))) & 0xffu);
}

// pass 1: per block and channel, the sum of the hue- and saturation-adjusted values of its (up to) 1024 pixels of image
// blockIdx.y, in a fixed order -> part[n][blockIdx.x][3].  Reads the pixels in storage order (the mean ignores the mirror).
// VEC: every image row holds a multiple of 4 pixels.
// (the body: `src` is the image, `part3` the block's 3 partial sums)
template <bool VEC>
__device__ __forceinline__ void rgb_aug_stats_block(const uint8_t* __restrict__ src, float* __restrict__ part3, int hw, float hue, float sat) {
    const int p0 = blockIdx.x * AUG_BLOCK_PIX + threadIdx.x * AUG_PIX;
    float acc[3] = {0.f, 0.f, 0.f};
    if (VEC && p0 < hw) {
        float px[12];
        load4px(src, p0, px);
#pragma unroll
        for (int j = 0; j < AUG_PIX; ++j) {
            hue_saturation(px[3 * j], px[3 * j + 1], px[3 * j + 2], hue, sat);
            acc[0] += px[3 * j]; acc[1] += px[3 * j + 1]; acc[2] += px[3 * j + 2];
        }
    } else if (!VEC) {
        for (int j = 0; j < AUG_PIX; ++j) {
            const int p = p0 + j;
            if (p >= hw) break;
            float r = src[p * 3], g = src[p * 3 + 1], b = src[p * 3 + 2];
            hue_saturation(r, g, b, hue, sat);
            acc[0] += r; acc[1] += g; acc[2] += b;
        }
    }
    __shared__ float red[AUG_THREADS / 64][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = wave_sum(acc[c]);
        if (lane == 0) red[wv][c] = t;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < AUG_THREADS / 64; ++k) t += red[k][threadIdx.x];
        part3[threadIdx.x] = t;
    }
}

template <bool VEC, typename SEL>
__global__ void __launch_bounds__(AUG_THREADS) rgb_stats_kernel(const uint8_t* __restrict__ src_img, SEL sel, float* __restrict__ part, int n0, int hw,
                                                                 float hue, float sat) {
    const int n = blockIdx.y;
    rgb_aug_stats_block<VEC>(src_img + sel.source(n0, n) * hw * 3, part + ((long long)(n0 + n) * gridDim.x + blockIdx.x) * 3, hw, hue, sat);
}

// pass 2: means[n][c] = (sum of the nb block partials, in double, fixed order) / hw.  One wave per (channel, image).
__global__ void __launch_bounds__(64) rgb_aug_means_kernel(const float* __restrict__ part, float* __restrict__ means, int nb, int hw) {
    const int c = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
    double t = 0.0;
    for (int k = lane; k < nb; k += 64) t += (double)part[((long long)n * nb + k) * 3 + c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) means[n * 3 + c] = (float)(t / (double)hw);
}

// pass 3: recompute the adjusted pixel from the uint8 input, contrast about the mean, brightness, clip; output pixel x of a
// flagged image comes from source pixel w - 1 - x
// (the body: `src` / `dst` are the image and its output, `mean3` its 3 means, `f` its flag)
template <bool VEC>
__device__ __forceinline__ void rgb_aug_apply_block(const uint8_t* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mean3,
                                                    bool f, int h, int w, float hue, float sat, float con, float bri) {
    const int hw = h * w;
    const float m0 = mean3[0], m1 = mean3[1], m2 = mean3[2];
    const int p0 = blockIdx.x * AUG_BLOCK_PIX + threadIdx.x * AUG_PIX;
    if (VEC) {
        if (p0 >= hw) return;
        // the 4 output pixels share a row (w % 4 == 0); mirrored, their sources are the 4 pixels ending at w - 1 - x, reversed
        const int y = p0 / w, x = p0 - y * w;
        float px[12];
        load4px(src, y * w + (f ? w - AUG_PIX - x : x), px);
        float o[12];
#pragma unroll
        for (int j = 0; j < AUG_PIX; ++j) {
            float r = px[3 * j], g = px[3 * j + 1], b = px[3 * j + 2];
            hue_saturation(r, g, b, hue, sat);
            const int k = f ? AUG_PIX - 1 - j : j;
            o[3 * k] = contrast_brightness(r, m0, con, bri);
            o[3 * k + 1] = contrast_brightness(g, m1, con, bri);
            o[3 * k + 2] = contrast_brightness(b, m2, con, bri);
        }
        float* d = dst + (long long)p0 * 3;
        st4(d, make_float4(o[0], o[1], o[2], o[3]));
        st4(d + 4, make_float4(o[4], o[5], o[6], o[7]));
        st4(d + 8, make_float4(o[8], o[9], o[10], o[11]));
    } else {
        for (int j = 0; j < AUG_PIX; ++j) {
            const int p = p0 + j;
            if (p >= hw) break;
            const int y = p / w, x = p - y * w;
            const int s = y * w + (f ? w - 1 - x : x);
            float r = src[s * 3], g = src[s * 3 + 1], b = src[s * 3 + 2];
            hue_saturation(r, g, b, hue, sat);
            dst[p * 3] = contrast_brightness(r, m0, con, bri);
            dst[p * 3 + 1] = contrast_brightness(g, m1, con, bri);
            dst[p * 3 + 2] = contrast_brightness(b, m2, con, bri);
        }
    }
}

template <bool VEC, typename SEL>
__global__ void __launch_bounds__(AUG_THREADS) rgb_apply_kernel(const uint8_t* __restrict__ src_img, SEL sel, const float* __restrict__ means,
                                                                 float* __restrict__ out, int n0, int h, int w, float hue, float sat, float con,
                                                                 float bri) {
    const int n = blockIdx.y;
    const long long img = (long long)h * w * 3;
    rgb_aug_apply_block<VEC>(src_img + sel.source(n0, n) * img, out + (n0 + n) * img, means + (n0 + n) * 3, sel.mirrored(n0, n), h, w, hue, sat, con,
                             bri);
}

// ---------------------------------------------------------------- cast + one-hot (read_and_encode's tensor part)
// one one-hot row: c floats, a 1 at class k (k >= c: none); c == 4 and a 16-byte aligned row is one float4 store
__device__ __forceinline__ void store_onehot(float* d, int k, int c) {
    if (c == 4 && ((uintptr_t)d & 15) == 0) {
        st4(d, make_float4(k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f, k == 3 ? 1.f : 0.f));
    } else {
        for (int t = 0; t < c; ++t) d[t] = k == t ? 1.f : 0.f;
    }
}

// one thread per OUTPUT pixel: 3 + 1 bytes in, 3 + c floats out (c <= 8); mirrored, its source is pixel w - 1 - x of its row.
// Either half may be NULL.  (No four-pixel form: with dword loads and 3 + c float4 stores per thread this pass measured 0.105 ms
// at 32 x 480 x 640, c = 4, against 0.075 ms for this one, where the stores of a wave are contiguous.)
template <typename SEL>
__global__ void __launch_bounds__(256) expand_kernel(const uint8_t* __restrict__ src_img, const uint8_t* __restrict__ src_midx, SEL sel,
                                                     float* __restrict__ out_img, float* __restrict__ out_mask, int n0, int h, int w, int c) {
    const int n = blockIdx.y, hw = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int y = p / w, x = p - y * w;
    const long long s = sel.source(n0, n) * hw + y * w + (sel.mirrored(n0, n) ? w - 1 - x : x);      // source pixel
    const long long o = (long long)(n0 + n) * hw + p;                                                // output pixel
    if (src_img != nullptr) {
        const uint8_t* r = src_img + s * 3;
        float* d = out_img + o * 3;
        d[0] = (float)r[0]; d[1] = (float)r[1]; d[2] = (float)r[2];
    }
    if (src_midx != nullptr) store_onehot(out_mask + o * c, src_midx[s], c);
}

// ground-truth rows and counts of gathered samples: every row written -- rows g < count of a flagged sample mirrored as
// flip_gt_boxes_kernel does, rows past the count zero
__global__ void __launch_bounds__(64) gather_gt_kernel(const float* __restrict__ pool_gt, const int32_t* __restrict__ pool_cnt, gather_sel sel,
                                                       float* __restrict__ gt, int32_t* __restrict__ gt_count, int n0, int gmax, float width) {
    const int n = blockIdx.y, g = blockIdx.x * 64 + threadIdx.x;
    if (g >= gmax) return;
    const long long s = sel.source(n0, n);
    const int cnt = pool_cnt[s];
    if (g == 0) gt_count[n0 + n] = cnt;
    const float* r = pool_gt + (s * gmax + g) * 5;             // (label, xmin, ymin, xmax, ymax)
    float* o = gt + ((long long)(n0 + n) * gmax + g) * 5;
    if (g < cnt) {
        float xmin = r[1], xmax = r[3];
        if (sel.mirrored(n0, n)) mirror_box(width, xmin, xmax);
        o[0] = r[0]; o[1] = xmin; o[2] = r[2]; o[3] = xmax; o[4] = r[4];
    } else {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
    }
}

// ---------------------------------------------------------------- host: each pass once, for either kind of batch
// `make(n0, count)` gives the selection (batch_sel.h) of output samples [n0, n0 + count); its type says how many one launch takes

template <typename MAKE>
int expand_pass(ssdseg_ctx* ctx, const uint8_t* src_img, const uint8_t* src_midx, MAKE make, float* out_img, float* out_mask, int b, int h, int w,
                int c) {
    using SEL = decltype(make(0, 0));
    const int hw = h * w;
    return for_each_chunk(b, SEL::chunk, [&](int n0, int count) {
        const double bytes = (double)count * hw * ((src_img ? 3.0 + 12.0 : 0.0) + (src_midx ? 1.0 + 4.0 * c : 0.0));
        SSDSEG_LAUNCH_NAMED(ctx, "expand_kernel", bytes, 0.0, expand_kernel<SEL>, dim3(cdiv(hw, 256), count), dim3(256), 0, src_img, src_midx,
                            make(n0, count), out_img, out_mask, n0, h, w, c);
        return launch_status("expand_kernel");
    });
}

// the three colour passes; the block partials of pass 1 live in the ctx workspace
template <typename MAKE>
int rgb_passes(ssdseg_ctx* ctx, const uint8_t* src_img, MAKE make, const float* draws4, float* means, float* out, int b, int h, int w) {
    using SEL = decltype(make(0, 0));
    // dword pixel loads and float4 stores: whole groups of 4 pixels per row and aligned buffers
    const bool vec = w % AUG_PIX == 0 && ((uintptr_t)src_img & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const float hue = draws4[0], sat = draws4[1], con = draws4[2], bri = draws4[3];
    const int hw = h * w, nb = cdiv(hw, AUG_BLOCK_PIX);
    void* ws = nullptr;
    int rc = ssdseg_workspace(ctx, (size_t)b * nb * 3 * sizeof(float), &ws);
    if (rc) return rc;
    float* part = static_cast<float*>(ws);
    rc = for_each_chunk(b, SEL::chunk, [&](int n0, int count) {
        return launch_vec<rgb_stats_kernel<true, SEL>, rgb_stats_kernel<false, SEL>>(ctx, vec, "rgb_stats_kernel", 3.0 * count * hw + 12.0 * count * nb,
                                                                                    dim3(nb, count), AUG_THREADS, src_img, make(n0, count), part, n0, hw,
                                                                                    hue, sat);
    });
    if (rc) return rc;
    rc = for_each_chunk(b, GRID_Y_MAX, [&](int n0, int count) {                 // one grid row per image
        SSDSEG_LAUNCH(ctx, 12.0 * count * nb + 12.0 * count, 0.0, rgb_aug_means_kernel, dim3(3, count), dim3(64), 0, part + (size_t)n0 * nb * 3,
                      means + (size_t)n0 * 3, nb, hw);
        return launch_status("rgb_aug_means_kernel");
    });
    if (rc) return rc;
    return for_each_chunk(b, SEL::chunk, [&](int n0, int count) {
        return launch_vec<rgb_apply_kernel<true, SEL>, rgb_apply_kernel<false, SEL>>(ctx, vec, "rgb_apply_kernel", 15.0 * count * hw + 12.0 * count,
                                                                                    dim3(nb, count), AUG_THREADS, src_img, make(n0, count), means, out, n0,
                                                                                    h, w, hue, sat, con, bri);
    });
}

}  // namespace

extern "C" {

int ssdseg_expand_inputs(ssdseg_ctx* ctx, const uint8_t* images_u8, const uint8_t* mask_index_u8, const uint8_t* flip, float* images_f32,
                         float* mask_onehot, int b, int h, int w, int c) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(images_u8 != nullptr || mask_index_u8 != nullptr, 2);
    SSDSEG_ARG(images_u8 == nullptr || images_f32 != nullptr, 5);
    SSDSEG_ARG(mask_index_u8 == nullptr || mask_onehot != nullptr, 6);
    SSDSEG_ARG(b > 0 && h > 0 && w > 0, 7);
    SSDSEG_ARG((long long)h * w * 3 < (1LL << 31), 8);       // in-image pixel and byte offsets in 32 bits
    SSDSEG_ARG(c > 0 && c <= 8, 10);
    return expand_pass(ctx, images_u8, mask_index_u8, [=](int, int) { return plain_sel{flip}; }, images_f32, mask_onehot, b, h, w, c);
}

int ssdseg_flip_gt_boxes(ssdseg_ctx* ctx, float* gt, const int32_t* gt_count, const uint8_t* flip, int b, int gmax, float image_width) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(gt != nullptr, 2);
    SSDSEG_ARG(gt_count != nullptr, 3);
    SSDSEG_ARG(flip != nullptr, 4);
    SSDSEG_ARG(b > 0 && gmax > 0, 5);
    SSDSEG_LAUNCH(ctx, 40.0 * b * gmax, 0.0, flip_gt_boxes_kernel, dim3(cdiv(b * gmax, 256)), dim3(256), 0, gt, gt_count, flip, b, gmax, image_width);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_rgb_augment(ssdseg_ctx* ctx, const uint8_t* images_u8, const uint8_t* flip, const float* draws4_host, float* means, float* images_f32,
                       int b, int h, int w) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(images_u8 != nullptr, 2);
    SSDSEG_ARG(draws4_host != nullptr, 4);
    SSDSEG_ARG(draws_finite(draws4_host), 4);
    SSDSEG_ARG(means != nullptr, 5);
    SSDSEG_ARG(images_f32 != nullptr, 6);
    SSDSEG_ARG(b > 0 && h > 0 && w > 0, 7);
    // one grid row per image; in-image pixel and byte offsets in 32 bits
    SSDSEG_ARG(b <= 65535 && (long long)h * w * 3 < (1LL << 31), 7);
    return rgb_passes(ctx, images_u8, [=](int, int) { return plain_sel{flip}; }, draws4_host, means, images_f32, b, h, w);
}

int ssdseg_gather_inputs(ssdseg_ctx* ctx, const uint8_t* pool_images, const uint8_t* pool_masks, int n_pool, const int32_t* index_host,
                         const uint8_t* flip_host, const float* draws4_host, float* means, float* images_f32, float* mask_onehot, int b, int h,
                         int w, int c) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(pool_images != nullptr || pool_masks != nullptr, 2);
    SSDSEG_ARG(n_pool > 0, 4);
    SSDSEG_ARG(index_host != nullptr, 5);
    SSDSEG_ARG(draws4_host == nullptr || pool_images != nullptr, 7);
    SSDSEG_ARG(draws4_host == nullptr || draws_finite(draws4_host), 7);
    SSDSEG_ARG(draws4_host == nullptr || means != nullptr, 8);
    SSDSEG_ARG(pool_images == nullptr || images_f32 != nullptr, 9);
    SSDSEG_ARG(pool_masks == nullptr || mask_onehot != nullptr, 10);
    SSDSEG_ARG(b > 0 && h > 0 && w > 0, 11);
    SSDSEG_ARG((long long)h * w * 3 < (1LL << 31), 12);      // in-image pixel and byte offsets in 32 bits
    SSDSEG_ARG(c > 0 && c <= 8, 14);
    SSDSEG_ARG(indices_in_source(index_host, b, n_pool), 5);
    const bool colour = draws4_host != nullptr;
    const auto make = [=](int n0, int count) { return make_sel(index_host, flip_host, n0, count); };
    // the plain expansion: both halves, or only the mask when the image comes from the colour passes
    const uint8_t* ex_img = colour ? nullptr : pool_images;
    if (ex_img != nullptr || pool_masks != nullptr) {
        const int rc = expand_pass(ctx, ex_img, pool_masks, make, images_f32, mask_onehot, b, h, w, c);
        if (rc) return rc;
    }
    return colour ? rgb_passes(ctx, pool_images, make, draws4_host, means, images_f32, b, h, w) : 0;
}

int ssdseg_gather_gt(ssdseg_ctx* ctx, const float* pool_gt, const int32_t* pool_cnt, int n_pool, const int32_t* index_host,
                     const uint8_t* flip_host, float* gt, int32_t* gt_count, int b, int gmax, float image_width) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(pool_gt != nullptr, 2);
    SSDSEG_ARG(pool_cnt != nullptr, 3);
    SSDSEG_ARG(n_pool > 0, 4);
    SSDSEG_ARG(index_host != nullptr, 5);
    SSDSEG_ARG(gt != nullptr, 7);
    SSDSEG_ARG(gt_count != nullptr, 8);
    SSDSEG_ARG(b > 0 && gmax > 0, 9);
    SSDSEG_ARG(indices_in_source(index_host, b, n_pool), 5);
    return for_each_chunk(b, gather_sel::chunk, [&](int n0, int count) {
        SSDSEG_LAUNCH(ctx, (40.0 * gmax + 8.0) * count, 0.0, gather_gt_kernel, dim3(cdiv(gmax, 64), count), dim3(64), 0, pool_gt, pool_cnt,
                      make_sel(index_host, flip_host, n0, count), gt, gt_count, n0, gmax, image_width);
        return launch_status("gather_gt_kernel");
    });
}

}  // extern "C"
