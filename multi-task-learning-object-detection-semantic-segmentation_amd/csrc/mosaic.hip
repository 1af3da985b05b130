// Device-side mosaic augmentation (the reference has none, so it is opt-in): every output sample is assembled from four source
// samples around a split point (px, py) -- the crop of csrc/crop.hip generalised to four (source, window) pairs per output sample,
// each with a destination rectangle (its quadrant) instead of the whole image.  It stands where the crop stands: in front of the
// flip and the colour augmentation of csrc/inputs.hip, uint8 -> uint8 into a dense compact batch.
//   quadrant k of an H x W sample:  0 top-left [0, px) x [0, py)   1 top-right [px, W) x [0, py)
//                                   2 bottom-left [0, px) x [py, H)   3 bottom-right [px, W) x [py, H)      (empty ones contribute nothing)
//   ssdseg_mosaic_inputs   pixels (bilinear, fill colour outside the source image) and class indices (nearest, fill class outside):
//                          tile k's window (x0, y0, w, h) of source index[k] mapped onto quadrant k;
//   ssdseg_mosaic_gt       the ground-truth rows of the four tiles whose centre lies in their window, scaled and shifted into the
//                          quadrant, clipped to it, compacted in visiting order (tile 0..3, the source's rows in their order).
// Float work: the host spec datacoder._mosaic_resample / _mosaic_gt operation for operation in float32 -- the tap arithmetic is
// that of the crop (crop_sample.h), this unit is built with -ffp-contract=off, and the only divisions, w / qw and qw / w, are done
// on the host, correctly rounded -- so it agrees with the spec byte for byte (tests/test_gpu_mosaic.py).  Indices, splits, windows
// and fill travel BY VALUE in the kernel arguments, 16 samples per launch (1.9 KB, the size of crop.hip's block of 64).
#include "batch_sel.h"
#include "crop_sample.h"

namespace {

struct mosaic_sel {
    static constexpr int chunk = 16;
    int32_t index[chunk][4];                 // the source sample of tile k
    int32_t split[chunk][2];                 // (px, py)
    float win[chunk][4][4];                  // tile k: (x0, y0, w, h)
    float scale[chunk][4][2];                // mosaic_inputs: (w / qw, h / qh); mosaic_gt: (qw / w, qh / h); 0 for an empty quadrant
    uint32_t flip;                           // bit n: the sample's flag, handed on to flip_out (the mosaic itself mirrors nothing)
    uint32_t fill;                           // r | g << 8 | b << 16 | fill_class << 24
};

// the parameters of one tile as a thread holds them (selected from the two tiles of its quadrant row, then per pixel)
struct tile_view {
    const uint8_t* img;
    const uint8_t* mask;
    float x0, sx;
    crop_rows rows;
};

// member by member, so that both stay in registers
__device__ __forceinline__ tile_view pick(bool first, const tile_view& a, const tile_view& b) {
    tile_view t;
    t.img = first ? a.img : b.img; t.mask = first ? a.mask : b.mask;
    t.x0 = first ? a.x0 : b.x0; t.sx = first ? a.sx : b.sx;
    t.rows.y0 = first ? a.rows.y0 : b.rows.y0; t.rows.y1 = first ? a.rows.y1 : b.rows.y1; t.rows.ym = first ? a.rows.ym : b.rows.ym;
    t.rows.in0 = first ? a.rows.in0 : b.rows.in0; t.rows.in1 = first ? a.rows.in1 : b.rows.in1; t.rows.inm = first ? a.rows.inm : b.rows.inm;
    t.rows.ay = first ? a.rows.ay : b.rows.ay;
    return t;
}

// VEC (w % 4 == 0, dword-aligned outputs): four consecutive output pixels of one row per thread, stored as 3 dwords of pixels and
// 1 dword of class indices; the four may straddle px, so the tile is chosen per pixel (the row lies in one quadrant row).  Otherwise
// one pixel per thread and byte stores.  blockIdx.y is the sample within the chunk.  The argument block is read with wave-uniform
// indices only (all four tiles, then selects): a lane-varying index would put it into scratch.
template <bool VEC>
__global__ void __launch_bounds__(256) mosaic_inputs_kernel(const uint8_t* __restrict__ src_img, const uint8_t* __restrict__ src_mask, mosaic_sel sel,
                                                            uint8_t* __restrict__ out_img, uint8_t* __restrict__ out_mask,
                                                            uint8_t* __restrict__ flip_out, int n0, int h, int w) {
    const int n = blockIdx.y, hw = h * w;
    if (flip_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) flip_out[n0 + n] = (uint8_t)((sel.flip >> n) & 1u);
    const int px = sel.split[n][0], py = sel.split[n][1];
    const float fill[3] = {(float)(sel.fill & 0xffu), (float)((sel.fill >> 8) & 0xffu), (float)((sel.fill >> 16) & 0xffu)};
    const uint32_t fill_class = sel.fill >> 24;
    const long long o = (long long)(n0 + n) * hw;          // first output pixel of this sample
    constexpr int PIX = VEC ? 4 : 1;
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * PIX;
    if (p0 >= hw) return;
    const int y = p0 / w, x = p0 - y * w;
    const bool lower = y >= py;
    const int oy = lower ? y - py : y;                     // the row within its quadrant
    tile_view side[2];                                     // the left and the right tile of this row
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long long s = lower ? sel.index[n][2 + j] : sel.index[n][j];
        const float wy0 = lower ? sel.win[n][2 + j][1] : sel.win[n][j][1];
        const float sy = lower ? sel.scale[n][2 + j][1] : sel.scale[n][j][1];
        side[j].img = src_img != nullptr ? src_img + s * hw * 3 : nullptr;
        side[j].mask = src_mask != nullptr ? src_mask + s * hw : nullptr;
        side[j].x0 = lower ? sel.win[n][2 + j][0] : sel.win[n][j][0];
        side[j].sx = lower ? sel.scale[n][2 + j][0] : sel.scale[n][j][0];
        side[j].rows = crop_row_setup(wy0, sy, oy, h);
    }
    uint32_t q[3 * PIX], m = 0;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const bool right = x + j >= px;
        const tile_view t = pick(right, side[1], side[0]);
        const float u = crop_centre(t.x0, right ? x + j - px : x + j, t.sx);
        if (src_img != nullptr) crop_pixel(t.img, t.rows, u, w, fill, q + 3 * j);
        if (src_mask != nullptr) m |= crop_class(t.mask, t.rows, u, w, fill_class) << (8 * j);
    }
    if constexpr (VEC) {
        if (src_img != nullptr) {
            uint32_t* d = reinterpret_cast<uint32_t*>(out_img + (o + p0) * 3);
            d[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            d[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
            d[2] = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
        }
        if (src_mask != nullptr) *reinterpret_cast<uint32_t*>(out_mask + o + p0) = m;
    } else {
        if (src_img != nullptr) {
            uint8_t* d = out_img + (o + p0) * 3;
            d[0] = (uint8_t)q[0]; d[1] = (uint8_t)q[1]; d[2] = (uint8_t)q[2];
        }
        if (src_mask != nullptr) out_mask[o + p0] = (uint8_t)m;
    }
}

// One wave per output sample.  Tiles in order 0..3 (empty quadrants skipped), the source's rows in groups of 64; the kept rows of a
// group go to base + (number of kept rows in lower lanes), with `base` running across groups and tiles: an ordered compaction
// (ssdseg_encode_targets is order-sensitive).  Only rows < gmax are stored; the count is min(total, gmax); rows past it are zeros.
// A tile that is the whole image seen through exactly (0, 0, W, H) copies its rows verbatim.
__global__ void __launch_bounds__(64) mosaic_gt_kernel(const float* __restrict__ src_gt, const int32_t* __restrict__ src_cnt, mosaic_sel sel,
                                                       float* __restrict__ gt, int32_t* __restrict__ gt_count, int n0, int gmax, int w, int h) {
#pragma clang fp contract(off)
    const int n = blockIdx.x, lane = threadIdx.x;
    const int px = sel.split[n][0], py = sel.split[n][1];
    float* out = gt + (long long)(n0 + n) * gmax * 5;
    int base = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qxi = (k & 1) ? px : 0, qyi = (k & 2) ? py : 0;
        const int qwi = (k & 1) ? w - px : px, qhi = (k & 2) ? h - py : py;
        if (qwi <= 0 || qhi <= 0) continue;                    // wave-uniform
        const long long s = sel.index[n][k];
        const float x0 = sel.win[n][k][0], y0 = sel.win[n][k][1], ww = sel.win[n][k][2], wh = sel.win[n][k][3];
        const float kx = sel.scale[n][k][0], ky = sel.scale[n][k][1];
        const float qx = (float)qxi, qy = (float)qyi, qx1 = qx + (float)qwi, qy1 = qy + (float)qhi;
        const bool identity = qwi == w && qhi == h && x0 == 0.f && y0 == 0.f && ww == (float)w && wh == (float)h;
        const float x1 = x0 + ww, y1 = y0 + wh;
        int cnt = src_cnt[s];
        cnt = cnt < 0 ? 0 : (cnt > gmax ? gmax : cnt);
        const float* rows = src_gt + s * gmax * 5;
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
                    xmin = fminf(fmaxf(qx + (xmin - x0) * kx, qx), qx1);
                    xmax = fminf(fmaxf(qx + (xmax - x0) * kx, qx), qx1);
                    ymin = fminf(fmaxf(qy + (ymin - y0) * ky, qy), qy1);
                    ymax = fminf(fmaxf(qy + (ymax - y0) * ky, qy), qy1);
                    keep = keep && xmax - xmin >= 1.f && ymax - ymin >= 1.f;
                }
            }
            const unsigned long long kept = __ballot(keep);
            const int row = base + __popcll(kept & ((1ull << lane) - 1ull));
            if (keep && row < gmax) {
                float* o = out + row * 5;
                o[0] = label; o[1] = xmin; o[2] = ymin; o[3] = xmax; o[4] = ymax;
            }
            base += __popcll(kept);
        }
    }
    if (base > gmax) base = gmax;
    for (int i = base * 5 + lane; i < gmax * 5; i += 64) out[i] = 0.f;
    if (lane == 0) gt_count[n0 + n] = base;
}

// every source position given and inside the source; every split inside the image
bool tiles_in_source(const int32_t* index4, int b, int n_src) {
    for (int i = 0; i < 4 * b; ++i)
        if (index4[i] < 0 || index4[i] >= n_src) return false;
    return true;
}

bool splits_in_image(const int32_t* split, int b, int h, int w) {
    for (int i = 0; i < b; ++i)
        if (split[2 * i] < 0 || split[2 * i] > w || split[2 * i + 1] < 0 || split[2 * i + 1] > h) return false;
    return true;
}

// samples [n0, n0 + count) of the host lists as one kernel-argument block; inverse: the scales of mosaic_gt
mosaic_sel make_mosaic_sel(const int32_t* index4, const int32_t* split, const float* win, int n0, int count, int h, int w, bool inverse,
                           uint32_t fill, const uint8_t* flip_host) {
    mosaic_sel sel;
    memset(&sel, 0, sizeof(sel));
    for (int i = 0; i < count; ++i) {
        const size_t n = (size_t)(n0 + i);
        const int px = split[2 * n], py = split[2 * n + 1];
        sel.split[i][0] = px; sel.split[i][1] = py;
        if (flip_host != nullptr && flip_host[n] != 0) sel.flip |= 1u << i;
        for (int k = 0; k < 4; ++k) {
            const float* q = win + 16 * n + 4 * k;
            const int qw = (k & 1) ? w - px : px, qh = (k & 2) ? h - py : py;
            sel.index[i][k] = index4[4 * n + k];
            for (int c = 0; c < 4; ++c) sel.win[i][k][c] = q[c];
            if (qw <= 0 || qh <= 0) continue;                  // an empty quadrant is never sampled: its scales stay 0
            sel.scale[i][k][0] = inverse ? (float)qw / q[2] : q[2] / (float)qw;
            sel.scale[i][k][1] = inverse ? (float)qh / q[3] : q[3] / (float)qh;
        }
    }
    sel.fill = fill;
    return sel;
}

}  // namespace

extern "C" {

int ssdseg_mosaic_inputs(ssdseg_ctx* ctx, const uint8_t* src_images, const uint8_t* src_masks, int n_src, const int32_t* index4_host,
                         const int32_t* split_host, const float* windows_host, const uint8_t* fill_rgb_host, int fill_class,
                         const uint8_t* flip_host, uint8_t* flip_out, uint8_t* images_u8, uint8_t* mask_index_u8, int b, int h, int w) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(src_images != nullptr || src_masks != nullptr, 2);
    SSDSEG_ARG(n_src > 0, 4);
    SSDSEG_ARG(index4_host != nullptr, 5);
    SSDSEG_ARG(split_host != nullptr, 6);
    SSDSEG_ARG(windows_host != nullptr, 7);
    SSDSEG_ARG(fill_class >= 0 && fill_class <= 255, 9);
    SSDSEG_ARG(flip_host == nullptr || flip_out != nullptr, 11);
    SSDSEG_ARG(src_images == nullptr || (images_u8 != nullptr && images_u8 != src_images), 12);
    SSDSEG_ARG(src_masks == nullptr || (mask_index_u8 != nullptr && mask_index_u8 != src_masks), 13);
    SSDSEG_ARG(b > 0 && h > 0 && w > 0, 14);
    // in-image pixel and byte offsets in 32 bits; 33 * the larger side (the reach of a window in range) far inside an int
    SSDSEG_ARG((long long)h * w * 3 < (1LL << 31) && h <= (1 << 24) && w <= (1 << 24), 15);
    SSDSEG_ARG(tiles_in_source(index4_host, b, n_src), 5);
    SSDSEG_ARG(splits_in_image(split_host, b, h, w), 6);
    SSDSEG_ARG(windows_in_range(windows_host, 4 * b, h, w), 7);
    const int hw = h * w;
    const uint32_t fill = pack_fill(fill_rgb_host, fill_class);
    // dword stores: whole groups of 4 pixels per row and dword-aligned outputs (the taps are byte gathers: no condition on the source)
    const bool vec = w % 4 == 0 && (src_images == nullptr || ((uintptr_t)images_u8 & 3) == 0) && (src_masks == nullptr || ((uintptr_t)mask_index_u8 & 3) == 0);
    const int gx = vec ? cdiv(hw, 1024) : cdiv(hw, 256);
    return for_each_chunk(b, mosaic_sel::chunk, [&](int n0, int count) {
        const double bytes = (double)count * hw * ((src_images ? 6.0 : 0.0) + (src_masks ? 2.0 : 0.0));
        return launch_vec<mosaic_inputs_kernel<true>, mosaic_inputs_kernel<false>>(
            ctx, vec, "mosaic_inputs_kernel", bytes, dim3(gx, count), 256, src_images, src_masks,
            make_mosaic_sel(index4_host, split_host, windows_host, n0, count, h, w, false, fill, flip_host), images_u8, mask_index_u8,
            flip_host != nullptr ? flip_out : nullptr, n0, h, w);
    });
}

int ssdseg_mosaic_gt(ssdseg_ctx* ctx, const float* src_gt, const int32_t* src_cnt, int n_src, const int32_t* index4_host,
                     const int32_t* split_host, const float* windows_host, float* gt, int32_t* gt_count, int b, int gmax, int h, int w) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(src_gt != nullptr, 2);
    SSDSEG_ARG(src_cnt != nullptr, 3);
    SSDSEG_ARG(n_src > 0, 4);
    SSDSEG_ARG(index4_host != nullptr, 5);
    SSDSEG_ARG(split_host != nullptr, 6);
    SSDSEG_ARG(windows_host != nullptr, 7);
    SSDSEG_ARG(gt != nullptr && gt != src_gt, 8);
    SSDSEG_ARG(gt_count != nullptr && gt_count != src_cnt, 9);
    SSDSEG_ARG(b > 0, 10);
    SSDSEG_ARG(gmax > 0, 11);
    SSDSEG_ARG(h > 0 && h <= (1 << 24), 12);
    SSDSEG_ARG(w > 0 && w <= (1 << 24), 13);
    SSDSEG_ARG(tiles_in_source(index4_host, b, n_src), 5);
    SSDSEG_ARG(splits_in_image(split_host, b, h, w), 6);
    SSDSEG_ARG(windows_in_range(windows_host, 4 * b, h, w), 7);
    return for_each_chunk(b, mosaic_sel::chunk, [&](int n0, int count) {
        SSDSEG_LAUNCH(ctx, (4 * 20.0 * gmax + 20.0 * gmax + 24.0) * count, 0.0, mosaic_gt_kernel, dim3(count), dim3(64), 0, src_gt, src_cnt,
                      make_mosaic_sel(index4_host, split_host, windows_host, n0, count, h, w, true, 0u, nullptr), gt, gt_count, n0, gmax, w, h);
        return launch_status("mosaic_gt_kernel");
    });
}

}  // extern "C"
