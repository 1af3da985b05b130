// IoU-family box regression loss of the SSD head (not in the reference): smooth_l1_weight * smooth-L1 + (1 - overlap term), the
// overlap term (IoU, GIoU or DIoU) taken between the DECODED target and predicted boxes of every box-carrying anchor, with the
// analytic gradient through the decode.  Definition, tie and clamp rules: include/ssdseg.h (ssdseg_loc_loss_iou) and the NumPy
// spec tests/_iou_loss_oracle.py, which this file follows comparison for comparison.
// House rules of losses.hip: per-block partials, a per-image fold in fixed order, a gradient pass that reads the folded count, no
// float atomics.
#include "box_terms.h"
#include "common.h"

#include <cmath>

namespace {

constexpr float KEPS = 1e-7f;
constexpr int BPI = 16;  // blocks per image in the per-anchor passes

struct IouParams {
    float4 sd;      // standard deviations of the offsets
    int kind;       // 0 IoU, 1 GIoU, 2 DIoU
    float lambda;   // smooth_l1_weight
};

// continuous box of one anchor: corners c -+ w/2 (no +1 / (w-1)/2 pixel convention), raw and clamped sizes, exp() of the size offsets
struct Box {
    float cx, cy, ex, ey, rw, rh, w, h, x0, y0, x1, y1;
};

__device__ __forceinline__ Box decode_box(float4 o, float4 an, float4 sd) {
    Box q;
    q.cx = o.x * sd.x * an.z + an.x;
    q.cy = o.y * sd.y * an.w + an.y;
    q.ex = expf(o.z * sd.z);
    q.ey = expf(o.w * sd.w);
    q.rw = (q.ex - 1.f) * an.z;
    q.rh = (q.ey - 1.f) * an.w;
    q.w = q.rw > 0.f ? q.rw : 0.f;
    q.h = q.rh > 0.f ? q.rh : 0.f;
    q.x0 = q.cx - q.w / 2.f; q.y0 = q.cy - q.h / 2.f;
    q.x1 = q.cx + q.w / 2.f; q.y1 = q.cy + q.h / 2.f;
    return q;
}

// one axis: intersection extent i, enclosing extent e, and d i / d p1 = di1, d i / d p0 = -di0, d e / d p1 = de1, d e / d p0 = -de0.
// Every min / max / clamp is ONE strict comparison; at a tie the derivative goes where the comparison sends the value.
struct Axis {
    float i, e, di1, di0, de1, de0;
};

__device__ __forceinline__ Axis axis_terms(float p0, float p1, float g0, float g1) {
    Axis x;
    const bool hi_lt = p1 < g1, lo_gt = p0 > g0;
    const float raw = (hi_lt ? p1 : g1) - (lo_gt ? p0 : g0);
    const bool pos = raw > 0.f;
    x.i = pos ? raw : 0.f;
    const bool hi_gt = p1 > g1, lo_lt = p0 < g0;
    x.e = (hi_gt ? p1 : g1) - (lo_lt ? p0 : g0);
    x.di1 = (pos && hi_lt) ? 1.f : 0.f;
    x.di0 = (pos && lo_gt) ? 1.f : 0.f;
    x.de1 = hi_gt ? 1.f : 0.f;
    x.de0 = lo_lt ? 1.f : 0.f;
    return x;
}

// the overlap term of one anchor; with GRAD its gradient w.r.t. the predicted offsets in *d
template <bool GRAD>
__device__ __forceinline__ float iou_term(float4 t, float4 p, float4 an, const IouParams& ip, float4* d) {
    const Box g = decode_box(t, an, ip.sd), q = decode_box(p, an, ip.sd);
    const Axis ax = axis_terms(q.x0, q.x1, g.x0, g.x1), ay = axis_terms(q.y0, q.y1, g.y0, g.y1);
    const float inter = ax.i * ay.i;
    const float uni = q.w * q.h + g.w * g.h - inter;
    const float ue = uni + KEPS;
    float term = 1.f - inter / ue;
    // gradients of the term w.r.t. I, the predicted area pw ph, ew, eh, pcx, pcy
    float g_i = -(ue + inter) / (ue * ue), g_ap = inter / (ue * ue);
    float g_ew = 0.f, g_eh = 0.f, g_cx = 0.f, g_cy = 0.f;
    if (ip.kind == 1) {
        const float enc = ax.e * ay.e;
        const float ee = enc + KEPS;
        term += (enc - uni) / ee;
        if (GRAD) {
            g_i += 1.f / ee;
            g_ap -= 1.f / ee;
            const float g_e = ue / (ee * ee);
            g_ew = g_e * ay.e;
            g_eh = g_e * ax.e;
        }
    } else if (ip.kind == 2) {
        const float dx = q.cx - g.cx, dy = q.cy - g.cy;
        const float rho = dx * dx + dy * dy;
        const float ce = ax.e * ax.e + ay.e * ay.e + KEPS;
        term += rho / ce;
        if (GRAD) {
            const float k = -2.f * rho / (ce * ce);
            g_ew = k * ax.e;
            g_eh = k * ay.e;
            g_cx = 2.f * dx / ce;
            g_cy = 2.f * dy / ce;
        }
    }
    if (GRAD) {
        const float g_iw = g_i * ay.i, g_ih = g_i * ax.i;
        const float g_x1 = g_iw * ax.di1 + g_ew * ax.de1;
        const float g_x0 = -(g_iw * ax.di0) - g_ew * ax.de0;
        const float g_y1 = g_ih * ay.di1 + g_eh * ay.de1;
        const float g_y0 = -(g_ih * ay.di0) - g_eh * ay.de0;
        const float g_w = g_ap * q.h + (g_x1 - g_x0) * 0.5f;
        const float g_h = g_ap * q.w + (g_y1 - g_y0) * 0.5f;
        d->x = (g_cx + g_x0 + g_x1) * (ip.sd.x * an.z);
        d->y = (g_cy + g_y0 + g_y1) * (ip.sd.y * an.w);
        d->z = q.rw > 0.f ? g_w * (ip.sd.z * an.z * q.ex) : 0.f;
        d->w = q.rh > 0.f ? g_h * (ip.sd.w * an.w * q.ey) : 0.f;
    }
    return term;
}

// pass 1: per-block partial sums (lambda * smooth-L1 + term over the box anchors, #box anchors); the count is a sum of 0 / 1 floats, exact
__global__ void __launch_bounds__(256) loc_iou_prep_kernel(const float* __restrict__ yb, const float* __restrict__ pb,
                                                           const float* __restrict__ anchors, int a, IouParams ip, float* __restrict__ partial) {
    __shared__ float red[256];
    const int img = blockIdx.y;
    const int chunk = (a + gridDim.x - 1) / gridDim.x;
    const int i0 = blockIdx.x * chunk, i1 = min(a, i0 + chunk);
    float acc[2] = {0.f, 0.f};
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const long long o = ((long long)img * a + i) * 4;
        const float4 t = ld4(yb + o), p = ld4(pb + o);
        if (has_box(t) != 0.f) {
            acc[0] += ip.lambda * sl1_sum(t, p) + iou_term<false>(t, p, ld4(anchors + (long long)i * 4), ip, nullptr);
            acc[1] += 1.f;
        }
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) {
        float* row = partial + ((long long)img * gridDim.x + blockIdx.x) * 2;
        row[0] = acc[0]; row[1] = acc[1];
    }
}

// per-image totals in fixed order, and the loss from them
__global__ void loc_iou_fold_kernel(const float* __restrict__ partial, int nblk, int b, float* __restrict__ img_stats, float* __restrict__ loc_loss) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= b) return;
    float s[2];
    for (int k = 0; k < 2; ++k) {
        s[k] = 0.f;
        for (int q = 0; q < nblk; ++q) s[k] += partial[((long long)img * nblk + q) * 2 + k];
        img_stats[img * 2 + k] = s[k];
    }
    if (loc_loss) loc_loss[img] = s[0] / fmaxf(s[1], 1.f);
}

// pass 2: d_boxes = loc_scale / max(#box anchors, 1) * (lambda * d smooth-L1 + d term), exact zeros for an anchor without a box
__global__ void __launch_bounds__(256) loc_iou_grad_kernel(const float* __restrict__ yb, const float* __restrict__ pb,
                                                           const float* __restrict__ anchors, int a, IouParams ip,
                                                           const float* __restrict__ img_stats, float loc_scale, float* __restrict__ d_boxes) {
    const int img = blockIdx.y;
    const int chunk = (a + gridDim.x - 1) / gridDim.x;
    const int i0 = blockIdx.x * chunk, i1 = min(a, i0 + chunk);
    const float sc = loc_scale / fmaxf(img_stats[img * 2 + 1], 1.f);
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const long long o = ((long long)img * a + i) * 4;
        const float4 t = ld4(yb + o), p = ld4(pb + o);
        float4 d = f4(0.f);
        if (has_box(t) != 0.f) {
            float4 dt;
            iou_term<true>(t, p, ld4(anchors + (long long)i * 4), ip, &dt);
            const float4 ds = sl1_grad(ip.lambda, t, p);
            d = make_float4(sc * (ds.x + dt.x), sc * (ds.y + dt.y), sc * (ds.z + dt.z), sc * (ds.w + dt.w));
        }
        st4(d_boxes + o, d);
    }
}

}  // namespace

extern "C" {

int ssdseg_loc_loss_iou(ssdseg_ctx* ctx, const float* y_boxes, const float* p_boxes, const float* anchors_centroids, const float* stds4_host,
                        int b, int a, int kind, float smooth_l1_weight, float loc_scale, float* loc_loss, float* d_boxes) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(y_boxes != nullptr, 2);
    SSDSEG_ARG(p_boxes != nullptr, 3);
    SSDSEG_ARG(anchors_centroids != nullptr, 4);
    SSDSEG_ARG(stds4_host != nullptr, 5);
    SSDSEG_ARG(b > 0 && b <= 65535, 6);   // the image is gridDim.y of the per-anchor passes
    SSDSEG_ARG(a > 0, 7);
    const long long n = (long long)b * a;
    SSDSEG_ARG(n < (1LL << 30), 6);
    SSDSEG_ARG(kind >= 0 && kind <= 2, 8);
    for (int k = 0; k < 4; ++k) SSDSEG_ARG(std::isfinite(stds4_host[k]) && stds4_host[k] > 0.f, 5);
    SSDSEG_ARG(std::isfinite(smooth_l1_weight) && smooth_l1_weight >= 0.f, 9);
    SSDSEG_ARG(std::isfinite(loc_scale), 10);
    IouParams ip;
    ip.sd = make_float4(stds4_host[0], stds4_host[1], stds4_host[2], stds4_host[3]);
    ip.kind = kind;
    ip.lambda = smooth_l1_weight;
    // workspace: partial[b][BPI][2] | img_stats[b][2]; every word of both is written before it is read
    const size_t o_stats = (size_t)b * BPI * 8, total = o_stats + (size_t)b * 8;
    void* ws;
    int rc = ssdseg_workspace(ctx, total, &ws);
    if (rc) return rc;
    float* partial = (float*)ws;
    float* img_stats = (float*)((char*)ws + o_stats);
    SSDSEG_LAUNCH(ctx, 32.0 * n + 16.0 * a, 0.0, loc_iou_prep_kernel, dim3(BPI, b), dim3(256), 0, y_boxes, p_boxes, anchors_centroids, a, ip, partial);
    SSDSEG_LAUNCH_CHECK();
    SSDSEG_LAUNCH(ctx, 0.0, 0.0, loc_iou_fold_kernel, dim3(cdiv(b, 64)), dim3(64), 0, partial, BPI, b, img_stats, loc_loss);
    SSDSEG_LAUNCH_CHECK();
    if (d_boxes) {
        SSDSEG_LAUNCH(ctx, 48.0 * n + 16.0 * a, 0.0, loc_iou_grad_kernel, dim3(BPI, b), dim3(256), 0, y_boxes, p_boxes, anchors_centroids, a, ip,
                      img_stats, loc_scale, d_boxes);
        SSDSEG_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
