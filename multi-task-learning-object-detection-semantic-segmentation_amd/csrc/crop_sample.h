// The sampling arithmetic the crop (crop.hip) and the mosaic (mosaic.hip) share, written once: the centre of an output pixel in
// source units, the source rows of an output row, the bilinear byte of the four taps, the nearest class index -- and the range a
// window has to lie in for their float -> int conversions.  Float32 in the order of the host spec (datacoder._crop_axis /
// _crop_resample), one rounding per operation: the pragmas keep FMA contraction off in here, and the units that include this
// header are built with -ffp-contract=off on top (csrc/Makefile).
#pragma once
#include <cmath>

#include "common.h"

// o + (i + 0.5) * s: the centre of output pixel i in source units
__device__ __forceinline__ float crop_centre(float o, int i, float s) {
#pragma clang fp contract(off)
    return o + ((float)i + 0.5f) * s;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the source rows of one output row: bilinear taps yf, yf + 1 (addresses clamped into the image, `in` says whether the row exists)
// and the nearest row of the mask
struct crop_rows {
    int y0, y1, ym;
    bool in0, in1, inm;
    float ay;
};

__device__ __forceinline__ crop_rows crop_row_setup(float wy0, float sy, int oy, int h) {
#pragma clang fp contract(off)
    crop_rows r;
    const float v = crop_centre(wy0, oy, sy);
    const float Y = v - 0.5f, yf = floorf(Y);
    r.ay = Y - yf;
    const int yi = (int)yf, ym = (int)floorf(v);
    r.in0 = yi >= 0 && yi < h;
    r.in1 = yi + 1 >= 0 && yi + 1 < h;
    r.inm = ym >= 0 && ym < h;
    r.y0 = clampi(yi, h - 1); r.y1 = clampi(yi + 1, h - 1); r.ym = clampi(ym, h - 1);
    return r;
}

// one output pixel: 3 bytes from the four taps.  Every address is clamped into the image first; the fill is selected afterwards.
__device__ __forceinline__ void crop_pixel(const uint8_t* __restrict__ src, const crop_rows& r, float u, int w, const float fill[3], uint32_t out[3]) {
#pragma clang fp contract(off)
    const float X = u - 0.5f, xf = floorf(X), ax = X - xf;
    const int xi = (int)xf;
    const bool inx0 = xi >= 0 && xi < w, inx1 = xi + 1 >= 0 && xi + 1 < w;
    const uint8_t* p00 = src + ((long long)r.y0 * w + clampi(xi, w - 1)) * 3;
    const uint8_t* p01 = src + ((long long)r.y0 * w + clampi(xi + 1, w - 1)) * 3;
    const uint8_t* p10 = src + ((long long)r.y1 * w + clampi(xi, w - 1)) * 3;
    const uint8_t* p11 = src + ((long long)r.y1 * w + clampi(xi + 1, w - 1)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a00 = (float)p00[c], a01 = (float)p01[c], a10 = (float)p10[c], a11 = (float)p11[c];
        const float t00 = r.in0 && inx0 ? a00 : fill[c], t01 = r.in0 && inx1 ? a01 : fill[c];
        const float t10 = r.in1 && inx0 ? a10 : fill[c], t11 = r.in1 && inx1 ? a11 : fill[c];
        const float top = t00 + (t01 - t00) * ax;
        const float bot = t10 + (t11 - t10) * ax;
        const float v = top + (bot - top) * r.ay;
        out[c] = (uint32_t)floorf(v + 0.5f);             // v lies between its taps: [0, 255]
    }
}

__device__ __forceinline__ uint32_t crop_class(const uint8_t* __restrict__ src, const crop_rows& r, float u, int w, uint32_t fill_class) {
    const int xm = (int)floorf(u);
    const uint32_t k = src[(long long)r.ym * w + clampi(xm, w - 1)];
    return r.inm && xm >= 0 && xm < w ? k : fill_class;
}

// every one of `count` windows (x0, y0, w, h) finite and inside the range that keeps each float -> int conversion above in range
static inline bool windows_in_range(const float* win, int count, int h, int w) {
    const float mw = 16.f * (float)w, mh = 16.f * (float)h;
    for (int i = 0; i < count; ++i) {
        const float* q = win + 4 * (size_t)i;
        if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]) && std::isfinite(q[3]))) return false;
        if (!(q[2] >= 1.f && q[2] <= mw && q[3] >= 1.f && q[3] <= mh)) return false;
        if (!(std::fabs(q[0]) <= mw && std::fabs(q[1]) <= mh)) return false;
    }
    return true;
}

// r | g << 8 | b << 16 | fill_class << 24; fill_rgb_host NULL: 0, 0, 0
static inline uint32_t pack_fill(const uint8_t* fill_rgb_host, int fill_class) {
    uint32_t fill = (uint32_t)fill_class << 24;
    if (fill_rgb_host != nullptr) fill |= (uint32_t)fill_rgb_host[0] | ((uint32_t)fill_rgb_host[1] << 8) | ((uint32_t)fill_rgb_host[2] << 16);
    return fill;
}
