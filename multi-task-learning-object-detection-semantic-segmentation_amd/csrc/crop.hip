// Device-side random crop / zoom-out augmentation (the SSD recipe's sampling; the reference has none, so it is opt-in): the
// geometric step in front of the flip and the colour augmentation of csrc/inputs.hip, for batches whose pixels the host never sees
// again (datacoder.ResidentDataset) and for compact batches alike.  A crop window is (x0, y0, w, h) in source-pixel units (pixel i
// covers [i, i + 1)), one per sample, and may reach outside the image (zoom-out); the output has the sample's own size.
//   ssdseg_crop_inputs   uint8 pixels (bilinear, fill colour outside the image) and uint8 class indices (nearest neighbour, fill
//                        class outside) of the windows, uint8 -> uint8 into a dense compact batch;
//   ssdseg_crop_gt       the ground-truth rows whose centre lies in the window, shifted, scaled, clipped, compacted in their order.
// What they write is an ordinary compact batch, so ssdseg_expand_inputs / ssdseg_rgb_augment / ssdseg_flip_gt_boxes /
// ssdseg_encode_targets run on it unchanged.  Float work: it follows the host spec datacoder._crop_resample / _crop_gt operation
// for operation in float32 (no FMA contraction -- this unit is built with -ffp-contract=off on top of the pragmas -- and the only
// divisions, w / W and W / w, are done on the host, correctly rounded), so it agrees with it byte for byte
// (tests/test_gpu_random_crop.py).  The source is a pool + a host index list, or a plain batch (index list NULL: n -> n); indices,
// windows and fill travel BY VALUE in the kernel arguments beside the gather_sel block of batch_sel.h, 64 samples per launch.
// The sampling arithmetic itself (pixel centre, row setup, bilinear byte, nearest class) is in crop_sample.h, shared with mosaic.hip.
#include "batch_sel.h"
#include "crop_sample.h"

namespace {

struct crop_sel {
    gather_sel who;                          // the source sample; its flag is handed on to flip_out (the crop itself mirrors nothing)
    float win[gather_sel::chunk][4];         // (x0, y0, w, h)
    float scale[gather_sel::chunk][2];       // crop_inputs: (sx, sy) = (w / W, h / H); crop_gt: (kx, ky) = (W / w, H / h)
    uint32_t fill;                           // r | g << 8 | b << 16 | fill_class << 24
};

// VEC (w % 4 == 0, dword-aligned outputs): four consecutive output pixels of one row per thread, stored as 3 dwords of pixels and
// 1 dword of class indices.  Otherwise one pixel per thread and byte stores.  blockIdx.y is the sample within the chunk.
template <bool VEC>
__global__ void __launch_bounds__(256) crop_inputs_kernel(const uint8_t* __restrict__ src_img, const uint8_t* __restrict__ src_mask, crop_sel sel,
                                                          uint8_t* __restrict__ out_img, uint8_t* __restrict__ out_mask, uint8_t* __restrict__ flip_out,
                                                          int n0, int h, int w) {
    const int n = blockIdx.y, hw = h * w;
    if (flip_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) flip_out[n0 + n] = (uint8_t)sel.who.mirrored(n0, n);
    const long long s = sel.who.source(n0, n);
    const float wx0 = sel.win[n][0], wy0 = sel.win[n][1], sx = sel.scale[n][0], sy = sel.scale[n][1];
    const float fill[3] = {(float)(sel.fill & 0xffu), (float)((sel.fill >> 8) & 0xffu), (float)((sel.fill >> 16) & 0xffu)};
    const uint32_t fill_class = sel.fill >> 24;
    const uint8_t* img = src_img != nullptr ? src_img + s * hw * 3 : nullptr;
    const uint8_t* mask = src_mask != nullptr ? src_mask + s * hw : nullptr;
    const long long o = (long long)(n0 + n) * hw;          // first output pixel of this sample
    constexpr int PIX = VEC ? 4 : 1;
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (p0 >= hw) return;
    const int y = p0 / w, x = p0 - y * w;
    const crop_rows r = crop_row_setup(wy0, sy, y, h);
    if (VEC) {
        float u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = crop_centre(wx0, x + j, sx);
        if (img != nullptr) {
            uint32_t q[12];
#pragma unroll
            for (int j = 0; j < 4; ++j) crop_pixel(img, r, u[j], w, fill, q + 3 * j);
            uint32_t* d = reinterpret_cast<uint32_t*>(out_img + (o + p0) * 3);
            d[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            d[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
            d[2] = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
        }
        if (mask != nullptr) {
            uint32_t m = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) m |= crop_class(mask, r, u[j], w, fill_class) << (8 * j);
            *reinterpret_cast<uint32_t*>(out_mask + o + p0) = m;
        }
    } else {
        const float u = crop_centre(wx0, x, sx);
        if (img != nullptr) {
            uint32_t q[3];
            crop_pixel(img, r, u, w, fill, q);
            uint8_t* d = out_img + (o + p0) * 3;
            d[0] = (uint8_t)q[0]; d[1] = (uint8_t)q[1]; d[2] = (uint8_t)q[2];
        }
        if (mask != nullptr) out_mask[o + p0] = (uint8_t)crop_class(mask, r, u, w, fill_class);
    }
}

// One wave per sample.  The kept rows of each group of 64 go to base + (number of kept rows in lower lanes): an ordered compaction
// (ssdseg_encode_targets is order-sensitive).  An identity window copies the rows verbatim.  Rows past the new count are zeros.
__global__ void __launch_bounds__(64) crop_gt_kernel(const float* __restrict__ src_gt, const int32_t* __restrict__ src_cnt, crop_sel sel,
                                                     float* __restrict__ gt, int32_t* __restrict__ gt_count, int n0, int gmax, float width, float height) {
#pragma clang fp contract(off)
    const int n = blockIdx.x, lane = threadIdx.x;
    const long long s = sel.who.source(n0, n);
    const float x0 = sel.win[n][0], y0 = sel.win[n][1], ww = sel.win[n][2], wh = sel.win[n][3], kx = sel.scale[n][0], ky = sel.scale[n][1];
    const bool identity = x0 == 0.f && y0 == 0.f && ww == width && wh == height;
    const float x1 = x0 + ww, y1 = y0 + wh;
    int cnt = src_cnt[s];
    cnt = cnt < 0 ? 0 : (cnt > gmax ? gmax : cnt);
    const float* rows = src_gt + s * gmax * 5;
    float* out = gt + (long long)(n0 + n) * gmax * 5;
    int base = 0;
    for (int g0 = 0; g0 < cnt; g0 += 64) {
        const int g = g0 + lane;
        bool keep = false;
        float label = 0.f, xmin = 0.f, ymin = 0.f, xmax = 0.f, ymax = 0.f;
        if (g < cnt) {
            const float* r = rows + g * 5;                     // (label, xmin, ymin, xmax, ymax)
            label = r[0]; xmin = r[1]; ymin = r[2]; xmax = r[3]; ymax = r[4];
            keep = true;
            if (!identity) {
                const float cx = (xmin + xmax) * 0.5f, cy = (ymin + ymax) * 0.5f;
                keep = x0 <= cx && cx < x1 && y0 <= cy && cy < y1;
                xmin = fminf(fmaxf((xmin - x0) * kx, 0.f), width);
                xmax = fminf(fmaxf((xmax - x0) * kx, 0.f), width);
                ymin = fminf(fmaxf((ymin - y0) * ky, 0.f), height);
                ymax = fminf(fmaxf((ymax - y0) * ky, 0.f), height);
                keep = keep && xmax - xmin >= 1.f && ymax - ymin >= 1.f;
            }
        }
        const unsigned long long kept = __ballot(keep);
        if (keep) {
            float* o = out + (base + __popcll(kept & ((1ull << lane) - 1ull))) * 5;
            o[0] = label; o[1] = xmin; o[2] = ymin; o[3] = xmax; o[4] = ymax;
        }
        base += __popcll(kept);
    }
    for (int i = base * 5 + lane; i < gmax * 5; i += 64) out[i] = 0.f;
    if (lane == 0) gt_count[n0 + n] = base;
}

// samples [n0, n0 + count) of the host lists as one kernel-argument block; inverse: the scales of crop_gt
crop_sel make_crop_sel(const int32_t* index_host, const float* win, int n0, int count, int h, int w, bool inverse, uint32_t fill,
                       const uint8_t* flip_host) {
    crop_sel sel;
    memset(&sel, 0, sizeof(sel));
    sel.who = make_sel(index_host, flip_host, n0, count);
    for (int i = 0; i < count; ++i) {
        const float* q = win + 4 * (size_t)(n0 + i);
        for (int k = 0; k < 4; ++k) sel.win[i][k] = q[k];
        sel.scale[i][0] = inverse ? (float)w / q[2] : q[2] / (float)w;
        sel.scale[i][1] = inverse ? (float)h / q[3] : q[3] / (float)h;
    }
    sel.fill = fill;
    return sel;
}

}  // namespace

extern "C" {

int ssdseg_crop_inputs(ssdseg_ctx* ctx, const uint8_t* src_images, const uint8_t* src_masks, int n_src, const int32_t* index_host,
                       const float* windows_host, const uint8_t* fill_rgb_host, int fill_class, const uint8_t* flip_host, uint8_t* flip_out,
                       uint8_t* images_u8, uint8_t* mask_index_u8, int b, int h, int w) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(src_images != nullptr || src_masks != nullptr, 2);
    SSDSEG_ARG(n_src > 0, 4);
    SSDSEG_ARG(windows_host != nullptr, 6);
    SSDSEG_ARG(fill_class >= 0 && fill_class <= 255, 8);
    SSDSEG_ARG(flip_host == nullptr || flip_out != nullptr, 10);
    SSDSEG_ARG(src_images == nullptr || (images_u8 != nullptr && images_u8 != src_images), 11);
    SSDSEG_ARG(src_masks == nullptr || (mask_index_u8 != nullptr && mask_index_u8 != src_masks), 12);
    SSDSEG_ARG(b > 0 && h > 0 && w > 0, 13);
    // in-image pixel and byte offsets in 32 bits; 33 * the larger side (the reach of a window in range) far inside an int
    SSDSEG_ARG((long long)h * w * 3 < (1LL << 31) && h <= (1 << 24) && w <= (1 << 24), 14);
    SSDSEG_ARG(indices_in_source(index_host, b, n_src), 5);
    SSDSEG_ARG(windows_in_range(windows_host, b, h, w), 6);
    const int hw = h * w;
    const uint32_t fill = pack_fill(fill_rgb_host, fill_class);
    // dword stores: whole groups of 4 pixels per row and dword-aligned outputs (the taps are byte gathers: no condition on the source)
    const bool vec = w % 4 == 0 && (src_images == nullptr || ((uintptr_t)images_u8 & 3) == 0) && (src_masks == nullptr || ((uintptr_t)mask_index_u8 & 3) == 0);
    const int gx = vec ? cdiv(hw, 1024) : cdiv(hw, 256);
    return for_each_chunk(b, gather_sel::chunk, [&](int n0, int count) {
        const double bytes = (double)count * hw * ((src_images ? 6.0 : 0.0) + (src_masks ? 2.0 : 0.0));
        return launch_vec<crop_inputs_kernel<true>, crop_inputs_kernel<false>>(
            ctx, vec, "crop_inputs_kernel", bytes, dim3(gx, count), 256, src_images, src_masks,
            make_crop_sel(index_host, windows_host, n0, count, h, w, false, fill, flip_host), images_u8, mask_index_u8,
            flip_host != nullptr ? flip_out : nullptr, n0, h, w);
    });
}

int ssdseg_crop_gt(ssdseg_ctx* ctx, const float* src_gt, const int32_t* src_cnt, int n_src, const int32_t* index_host, const float* windows_host,
                   float* gt, int32_t* gt_count, int b, int gmax, int h, int w) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(src_gt != nullptr, 2);
    SSDSEG_ARG(src_cnt != nullptr, 3);
    SSDSEG_ARG(n_src > 0, 4);
    SSDSEG_ARG(windows_host != nullptr, 6);
    SSDSEG_ARG(gt != nullptr && gt != src_gt, 7);
    SSDSEG_ARG(gt_count != nullptr, 8);
    SSDSEG_ARG(b > 0 && gmax > 0, 9);
    SSDSEG_ARG(h > 0 && w > 0 && h <= (1 << 24) && w <= (1 << 24), 11);
    SSDSEG_ARG(indices_in_source(index_host, b, n_src), 5);
    SSDSEG_ARG(windows_in_range(windows_host, b, h, w), 6);
    return for_each_chunk(b, gather_sel::chunk, [&](int n0, int count) {
        SSDSEG_LAUNCH(ctx, (40.0 * gmax + 8.0) * count, 0.0, crop_gt_kernel, dim3(count), dim3(64), 0, src_gt, src_cnt,
                      make_crop_sel(index_host, windows_host, n0, count, h, w, true, 0u, nullptr), gt, gt_count, n0, gmax, (float)w, (float)h);
        return launch_status("crop_gt_kernel");
    });
}

}  // extern "C"
