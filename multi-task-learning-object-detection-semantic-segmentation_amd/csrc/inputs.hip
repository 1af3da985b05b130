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
#include <cmath>

#include "common.h"

namespace {

// one thread per OUTPUT pixel: 3 bytes + 1 byte in, 3 + c floats out (c <= 8; the one-hot row as float4 stores when c == 4)
__global__ void __launch_bounds__(256) expand_inputs_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ midx, const uint8_t* __restrict__ flip,
                                                            float* __restrict__ out_img, float* __restrict__ out_mask, int h, int w, int c,
                                                            long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % w);
        const long long row = i / w;                 // (image, y)
        const int n = (int)(row / h);
        const bool f = flip != nullptr && flip[n] != 0;
        const long long src = row * w + (f ? w - 1 - x : x);
        if (img != nullptr) {
            const uint8_t* p = img + src * 3;
            float* o = out_img + i * 3;
            o[0] = (float)p[0]; o[1] = (float)p[1]; o[2] = (float)p[2];
        }
        if (midx != nullptr) {
            const int k = midx[src];
            float* o = out_mask + i * c;
            if (c == 4) {
                st4(o, make_float4(k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f, k == 3 ? 1.f : 0.f));
            } else {
                for (int j = 0; j < c; ++j) o[j] = k == j ? 1.f : 0.f;
            }
        }
    }
}

__global__ void flip_gt_boxes_kernel(float* __restrict__ gt, const int* __restrict__ count, const uint8_t* __restrict__ flip, int b, int gmax,
                                     float width) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // over b * gmax rows
    if (i >= b * gmax) return;
    const int n = i / gmax, g = i - n * gmax;
    if (flip[n] == 0 || g >= count[n]) return;
    float* r = gt + (long long)i * 5;                          // (label, xmin, ymin, xmax, ymax)
    const float xmin = r[1], xmax = r[3];
    r[1] = width - xmax;
    r[3] = width - xmin;
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
// (the body, shared with the gathering form below: `src` is the image, `part3` the block's 3 partial sums)
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

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) rgb_aug_stats_kernel(const uint8_t* __restrict__ img, float* __restrict__ part, int hw,
                                                                     float hue, float sat) {
    const int n = blockIdx.y;
    rgb_aug_stats_block<VEC>(img + (long long)n * hw * 3, part + ((long long)n * gridDim.x + blockIdx.x) * 3, hw, hue, sat);
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
// (the body, shared with the gathering form below: `src` / `dst` are the image and its output, `mean3` its 3 means, `f` its flag)
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

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) rgb_aug_apply_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ flip,
                                                                     const float* __restrict__ means, float* __restrict__ out, int h, int w,
                                                                     float hue, float sat, float con, float bri) {
    const int n = blockIdx.y;
    const long long off = (long long)n * h * w * 3;
    rgb_aug_apply_block<VEC>(img + off, out + off, means + n * 3, flip != nullptr && flip[n] != 0, h, w, hue, sat, con, bri);
}

// ---------------------------------------------------------------- device-resident training set (datacoder.ResidentDataset)
// The samples stay in HBM as the files hold them (pools of uint8 pixels, uint8 class indices, ground-truth rows); a batch is a
// list of sample indices + flip flags drawn on the host each epoch (NB03#cell8: shuffle, read_and_encode, batch).  The list
// travels BY VALUE in the kernel arguments, GATHER_CHUNK samples per launch: no host -> device copy of its own, nothing the
// caller could overwrite while it is in flight, no synchronisation.  blockIdx.y is the sample within the chunk (wave-uniform
// reads of the argument block); all pool offsets are 64-bit (index * h * w * 3 passes 2^32 at 4,661 samples of 480x640).
constexpr int GATHER_CHUNK = 64;
struct gather_sel {
    int32_t index[GATHER_CHUNK];     // pool sample of output sample n0 + n
    unsigned long long flip;         // bit n: mirror it
};

// ssdseg_expand_inputs' work on gathered samples.  VEC (w % 4 == 0, aligned buffers): four consecutive output pixels per thread
// -- 3 dwords of pixels + 1 dword of class indices in, 3 + c float4 out; mirrored, they are the 4 source pixels ending at
// w - 1 - x, reversed.  Otherwise one pixel per thread, as expand_inputs_kernel.
template <bool VEC>
__global__ void __launch_bounds__(256) gather_expand_kernel(const uint8_t* __restrict__ pool_img, const uint8_t* __restrict__ pool_midx,
                                                            gather_sel sel, float* __restrict__ out_img, float* __restrict__ out_mask, int n0, int h,
                                                            int w, int c) {
    const int n = blockIdx.y, hw = h * w;
    const long long s = sel.index[n];
    const bool f = ((sel.flip >> n) & 1ull) != 0;
    const long long o = (long long)(n0 + n) * hw;          // first output pixel of this sample
    if (VEC) {
        const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
        if (p0 >= hw) return;
        const int y = p0 / w, x = p0 - y * w;
        const int sp = y * w + (f ? w - 4 - x : x);
        if (pool_img != nullptr) {
            float px[12], q[12];
            load4px(pool_img + s * hw * 3, sp, px);
#pragma unroll
            for (int j = 0; j < 12; ++j) q[j] = f ? px[3 * (3 - j / 3) + j % 3] : px[j];
            float* d = out_img + (o + p0) * 3;
            st4(d, make_float4(q[0], q[1], q[2], q[3]));
            st4(d + 4, make_float4(q[4], q[5], q[6], q[7]));
            st4(d + 8, make_float4(q[8], q[9], q[10], q[11]));
        }
        if (pool_midx != nullptr) {
            uint32_t m = *reinterpret_cast<const uint32_t*>(pool_midx + s * hw + sp);
            if (f) m = __builtin_bswap32(m);
            float* d = out_mask + (o + p0) * c;
            if (c == 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = (int)((m >> (8 * j)) & 0xffu);
                    st4(d + 4 * j, make_float4(k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f, k == 3 ? 1.f : 0.f));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = (int)((m >> (8 * j)) & 0xffu);
                    for (int t = 0; t < c; ++t) d[j * c + t] = k == t ? 1.f : 0.f;
                }
            }
        }
    } else {
        const int p = blockIdx.x * 256 + threadIdx.x;
        if (p >= hw) return;
        const int y = p / w, x = p - y * w;
        const int sp = y * w + (f ? w - 1 - x : x);
        if (pool_img != nullptr) {
            const uint8_t* r = pool_img + (s * hw + sp) * 3;
            float* d = out_img + (o + p) * 3;
            d[0] = (float)r[0]; d[1] = (float)r[1]; d[2] = (float)r[2];
        }
        if (pool_midx != nullptr) {
            const int k = pool_midx[s * hw + sp];
            float* d = out_mask + (o + p) * c;
            for (int t = 0; t < c; ++t) d[t] = k == t ? 1.f : 0.f;
        }
    }
}

// ssdseg_rgb_augment's passes 1 and 3 on gathered samples: the same block bodies on the same pixels, so the same partial sums,
// the same means (pass 2 is rgb_aug_means_kernel itself, once for the batch) and the same output bits
template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) gather_rgb_stats_kernel(const uint8_t* __restrict__ pool_img, gather_sel sel, float* __restrict__ part,
                                                                        int n0, int hw, float hue, float sat) {
    const int n = blockIdx.y;
    rgb_aug_stats_block<VEC>(pool_img + (long long)sel.index[n] * hw * 3, part + ((long long)(n0 + n) * gridDim.x + blockIdx.x) * 3, hw, hue, sat);
}

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) gather_rgb_apply_kernel(const uint8_t* __restrict__ pool_img, gather_sel sel,
                                                                        const float* __restrict__ means, float* __restrict__ out, int n0, int h, int w,
                                                                        float hue, float sat, float con, float bri) {
    const int n = blockIdx.y;
    rgb_aug_apply_block<VEC>(pool_img + (long long)sel.index[n] * h * w * 3, out + (long long)(n0 + n) * h * w * 3, means + (n0 + n) * 3,
                             ((sel.flip >> n) & 1ull) != 0, h, w, hue, sat, con, bri);
}

// ground-truth rows and counts of the gathered samples; rows g < count of a flagged sample mirrored as flip_gt_boxes_kernel does,
// rows past the count zero
__global__ void __launch_bounds__(64) gather_gt_kernel(const float* __restrict__ pool_gt, const int32_t* __restrict__ pool_cnt, gather_sel sel,
                                                       float* __restrict__ gt, int32_t* __restrict__ gt_count, int n0, int gmax, float width) {
    const int n = blockIdx.y, g = blockIdx.x * 64 + threadIdx.x;
    if (g >= gmax) return;
    const long long s = sel.index[n];
    const bool f = ((sel.flip >> n) & 1ull) != 0;
    const int cnt = pool_cnt[s];
    if (g == 0) gt_count[n0 + n] = cnt;
    const float* r = pool_gt + (s * gmax + g) * 5;             // (label, xmin, ymin, xmax, ymax)
    float* o = gt + ((long long)(n0 + n) * gmax + g) * 5;
    if (g < cnt) {
        const float xmin = r[1], xmax = r[3];
        o[0] = r[0];
        o[1] = f ? width - xmax : xmin;
        o[2] = r[2];
        o[3] = f ? width - xmin : xmax;
        o[4] = r[4];
    } else {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
    }
}

// samples [n0, n0 + count) of the host lists as one kernel-argument block
gather_sel make_sel(const int32_t* index_host, const uint8_t* flip_host, int n0, int count) {
    gather_sel sel;
    memset(&sel, 0, sizeof(sel));
    for (int i = 0; i < count; ++i) {
        sel.index[i] = index_host[n0 + i];
        if (flip_host != nullptr && flip_host[n0 + i] != 0) sel.flip |= 1ull << i;
    }
    return sel;
}

bool indices_in_pool(const int32_t* index_host, int b, int n_pool) {
    for (int i = 0; i < b; ++i)
        if (index_host[i] < 0 || index_host[i] >= n_pool) return false;
    return true;
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
    SSDSEG_ARG(c > 0 && c <= 8, 10);
    const long long total = (long long)b * h * w;
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    const double bytes = (double)total * ((images_u8 ? 3.0 + 12.0 : 0.0) + (mask_index_u8 ? 1.0 + 4.0 * c : 0.0));
    SSDSEG_LAUNCH(ctx, bytes, 0.0, expand_inputs_kernel, dim3(blocks), dim3(256), 0, images_u8, mask_index_u8, flip, images_f32, mask_onehot, h, w, c,
                  total);
    SSDSEG_LAUNCH_CHECK();
    return 0;
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
    SSDSEG_ARG(std::isfinite(draws4_host[0]) && std::isfinite(draws4_host[1]) && std::isfinite(draws4_host[2]) && std::isfinite(draws4_host[3]), 4);
    SSDSEG_ARG(means != nullptr, 5);
    SSDSEG_ARG(images_f32 != nullptr, 6);
    SSDSEG_ARG(b > 0 && h > 0 && w > 0, 7);
    // one grid row per image; in-image pixel and byte offsets in 32 bits
    SSDSEG_ARG(b <= 65535 && (long long)h * w * 3 < (1LL << 31), 7);
    const float hue = draws4_host[0], sat = draws4_host[1], con = draws4_host[2], bri = draws4_host[3];
    const int hw = h * w, nb = cdiv(hw, AUG_BLOCK_PIX);
    void* ws = nullptr;
    int rc = ssdseg_workspace(ctx, (size_t)b * nb * 3 * sizeof(float), &ws);
    if (rc) return rc;
    float* part = static_cast<float*>(ws);
    const double px = (double)b * hw;
    // dword pixel loads and float4 stores: whole groups of 4 pixels per row and aligned buffers
    const bool vec = w % AUG_PIX == 0 && ((uintptr_t)images_u8 & 3) == 0 && ((uintptr_t)images_f32 & 15) == 0;
    if (vec)
        SSDSEG_LAUNCH(ctx, 3.0 * px + 12.0 * b * nb, 0.0, rgb_aug_stats_kernel<true>, dim3(nb, b), dim3(AUG_THREADS), 0, images_u8, part, hw, hue, sat);
    else
        SSDSEG_LAUNCH(ctx, 3.0 * px + 12.0 * b * nb, 0.0, rgb_aug_stats_kernel<false>, dim3(nb, b), dim3(AUG_THREADS), 0, images_u8, part, hw, hue, sat);
    SSDSEG_LAUNCH_CHECK();
    SSDSEG_LAUNCH(ctx, 12.0 * b * nb + 12.0 * b, 0.0, rgb_aug_means_kernel, dim3(3, b), dim3(64), 0, part, means, nb, hw);
    SSDSEG_LAUNCH_CHECK();
    if (vec)
        SSDSEG_LAUNCH(ctx, 15.0 * px + 12.0 * b, 0.0, rgb_aug_apply_kernel<true>, dim3(nb, b), dim3(AUG_THREADS), 0, images_u8, flip, means, images_f32,
                      h, w, hue, sat, con, bri);
    else
        SSDSEG_LAUNCH(ctx, 15.0 * px + 12.0 * b, 0.0, rgb_aug_apply_kernel<false>, dim3(nb, b), dim3(AUG_THREADS), 0, images_u8, flip, means, images_f32,
                      h, w, hue, sat, con, bri);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_gather_inputs(ssdseg_ctx* ctx, const uint8_t* pool_images, const uint8_t* pool_masks, int n_pool, const int32_t* index_host,
                         const uint8_t* flip_host, const float* draws4_host, float* means, float* images_f32, float* mask_onehot, int b, int h,
                         int w, int c) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(pool_images != nullptr || pool_masks != nullptr, 2);
    SSDSEG_ARG(n_pool > 0, 4);
    SSDSEG_ARG(index_host != nullptr, 5);
    SSDSEG_ARG(draws4_host == nullptr || pool_images != nullptr, 7);
    SSDSEG_ARG(draws4_host == nullptr ||
               (std::isfinite(draws4_host[0]) && std::isfinite(draws4_host[1]) && std::isfinite(draws4_host[2]) && std::isfinite(draws4_host[3])), 7);
    SSDSEG_ARG(draws4_host == nullptr || means != nullptr, 8);
    SSDSEG_ARG(pool_images == nullptr || images_f32 != nullptr, 9);
    SSDSEG_ARG(pool_masks == nullptr || mask_onehot != nullptr, 10);
    SSDSEG_ARG(b > 0 && h > 0 && w > 0, 11);
    SSDSEG_ARG((long long)h * w * 3 < (1LL << 31), 12);      // in-image pixel and byte offsets in 32 bits
    SSDSEG_ARG(c > 0 && c <= 8, 14);
    SSDSEG_ARG(indices_in_pool(index_host, b, n_pool), 5);
    const int hw = h * w;
    const bool colour = draws4_host != nullptr;
    // dword loads and float4 stores: whole groups of 4 pixels per row and aligned buffers
    const bool vec = w % 4 == 0 && (pool_images == nullptr || (((uintptr_t)pool_images & 3) == 0 && ((uintptr_t)images_f32 & 15) == 0)) &&
                     (pool_masks == nullptr || (((uintptr_t)pool_masks & 3) == 0 && ((uintptr_t)mask_onehot & 15) == 0));
    const int nb = cdiv(hw, AUG_BLOCK_PIX);
    float hue = 0.f, sat = 1.f, con = 1.f, bri = 0.f;
    float* part = nullptr;
    if (colour) {
        hue = draws4_host[0]; sat = draws4_host[1]; con = draws4_host[2]; bri = draws4_host[3];
        void* ws = nullptr;
        int rc = ssdseg_workspace(ctx, (size_t)b * nb * 3 * sizeof(float), &ws);
        if (rc) return rc;
        part = static_cast<float*>(ws);
    }
    // the plain expansion: both halves, or only the mask when the image comes from the colour passes
    const uint8_t* ex_img = colour ? nullptr : pool_images;
    if (ex_img != nullptr || pool_masks != nullptr) {
        const int gx = vec ? cdiv(hw, 1024) : cdiv(hw, 256);
        for (int n0 = 0; n0 < b; n0 += GATHER_CHUNK) {
            const int count = b - n0 < GATHER_CHUNK ? b - n0 : GATHER_CHUNK;
            const gather_sel sel = make_sel(index_host, flip_host, n0, count);
            const double bytes = (double)count * hw * ((ex_img ? 3.0 + 12.0 : 0.0) + (pool_masks ? 1.0 + 4.0 * c : 0.0));
            if (vec)
                SSDSEG_LAUNCH(ctx, bytes, 0.0, gather_expand_kernel<true>, dim3(gx, count), dim3(256), 0, ex_img, pool_masks, sel, images_f32, mask_onehot,
                              n0, h, w, c);
            else
                SSDSEG_LAUNCH(ctx, bytes, 0.0, gather_expand_kernel<false>, dim3(gx, count), dim3(256), 0, ex_img, pool_masks, sel, images_f32,
                              mask_onehot, n0, h, w, c);
            SSDSEG_LAUNCH_CHECK();
        }
    }
    if (!colour) return 0;
    for (int n0 = 0; n0 < b; n0 += GATHER_CHUNK) {
        const int count = b - n0 < GATHER_CHUNK ? b - n0 : GATHER_CHUNK;
        const gather_sel sel = make_sel(index_host, nullptr, n0, count);       // the mean ignores the mirror
        const double bytes = 3.0 * count * hw + 12.0 * count * nb;
        if (vec)
            SSDSEG_LAUNCH(ctx, bytes, 0.0, gather_rgb_stats_kernel<true>, dim3(nb, count), dim3(AUG_THREADS), 0, pool_images, sel, part, n0, hw, hue, sat);
        else
            SSDSEG_LAUNCH(ctx, bytes, 0.0, gather_rgb_stats_kernel<false>, dim3(nb, count), dim3(AUG_THREADS), 0, pool_images, sel, part, n0, hw, hue, sat);
        SSDSEG_LAUNCH_CHECK();
    }
    for (int n0 = 0; n0 < b; n0 += 65535) {                                     // one grid row per image
        const int count = b - n0 < 65535 ? b - n0 : 65535;
        SSDSEG_LAUNCH(ctx, 12.0 * count * nb + 12.0 * count, 0.0, rgb_aug_means_kernel, dim3(3, count), dim3(64), 0, part + (size_t)n0 * nb * 3,
                      means + (size_t)n0 * 3, nb, hw);
        SSDSEG_LAUNCH_CHECK();
    }
    for (int n0 = 0; n0 < b; n0 += GATHER_CHUNK) {
        const int count = b - n0 < GATHER_CHUNK ? b - n0 : GATHER_CHUNK;
        const gather_sel sel = make_sel(index_host, flip_host, n0, count);
        const double bytes = 15.0 * count * hw + 12.0 * count;
        if (vec)
            SSDSEG_LAUNCH(ctx, bytes, 0.0, gather_rgb_apply_kernel<true>, dim3(nb, count), dim3(AUG_THREADS), 0, pool_images, sel, means, images_f32, n0,
                          h, w, hue, sat, con, bri);
        else
            SSDSEG_LAUNCH(ctx, bytes, 0.0, gather_rgb_apply_kernel<false>, dim3(nb, count), dim3(AUG_THREADS), 0, pool_images, sel, means, images_f32, n0,
                          h, w, hue, sat, con, bri);
        SSDSEG_LAUNCH_CHECK();
    }
    return 0;
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
    SSDSEG_ARG(indices_in_pool(index_host, b, n_pool), 5);
    for (int n0 = 0; n0 < b; n0 += GATHER_CHUNK) {
        const int count = b - n0 < GATHER_CHUNK ? b - n0 : GATHER_CHUNK;
        const gather_sel sel = make_sel(index_host, flip_host, n0, count);
        SSDSEG_LAUNCH(ctx, (40.0 * gmax + 8.0) * count, 0.0, gather_gt_kernel, dim3(cdiv(gmax, 64), count), dim3(64), 0, pool_gt, pool_cnt, sel, gt,
                      gt_count, n0, gmax, image_width);
        SSDSEG_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
