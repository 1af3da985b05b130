// Tail kernels of the SSDLite head and the anchor metrics (HBM-bound, float4 granules):
//   SSD head gather: Reshape(-1,4) + Concatenate(axis=1) (blocks.py:155, models.py:256,271) and Softmax (models.py:259)
//   weighted label accuracy and mean box IoU of the anchors (metrics.py:76-216)
#include "lerp_softmax.h"

namespace {

// ------------------------------------------------------------------------------------------------ SSD head gather / softmax
// forward: out[b][off + r] = view(in)[b][r], r in [0, in_img_elems), channel of element = r % c (float4 granules)
// reverse: in_grad[b][r] = out_grad[b][off + r]
__global__ void head_gather_kernel(const float* __restrict__ src, const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                   float* __restrict__ dst, int b, int in_img_elems, int c, int out_off, int out_img_elems, int reverse) {
    const int per = in_img_elems / 4;
    const long long total = (long long)b * per;
    const bool aff = scale != nullptr;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long img = i / per;
        const int r = (int)(i % per) * 4;
        const long long dense = img * in_img_elems + r, strided = img * out_img_elems + out_off + r;
        if (!reverse) {
            float4 s = f4(0.f), t = f4(0.f);
            const int c0 = r % c;
            if (aff) { s = ld4(scale + c0); t = ld4(shift + c0); }
            float4 v = ld4(src + dense);
            if (aff || act != SSDSEG_ACT_NONE) v = view_apply4(v, s, t, aff, act);   // a plain move keeps the bits: fma(1, -0.f, 0.f) is +0.f
            st4(dst + strided, v);
        } else {
            st4(dst + dense, ld4(src + strided));
        }
    }
}

__global__ void softmax_rows4_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                     float* __restrict__ out, long long rows) {
    const bool aff = scale != nullptr;
    float4 s = f4(0.f), t = f4(0.f);
    if (aff) { s = ld4(scale); t = ld4(shift); }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long long)gridDim.x * blockDim.x)
        st4(out + i * 4, softmax4(view_apply4(ld4(x + i * 4), s, t, aff, act)));
}

// ------------------------------------------------------------------------------------------------ training metrics
// (reference metrics.py; per-image values, Keras averages them).  All float reductions are two-level in fixed order.

// weighted "categorical accuracy" of the anchor labels (metrics.py:204-216): per class the number of anchors where
// one_hot(argmax p)[c] == y_true[c] (agreeing zeros count too), / #anchors, weighted sum.  One block per image, integer counts.
__global__ void __launch_bounds__(256) label_accuracy_kernel(const float* __restrict__ y_true, const float* __restrict__ y_pred, int a,
                                                             float4 cw, float* __restrict__ out) {
    __shared__ int red[4][256];
    const int img = blockIdx.x;
    int cnt[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < a; i += 256) {
        const float4 t = ld4(y_true + ((long long)img * a + i) * 4), p = ld4(y_pred + ((long long)img * a + i) * 4);
        int am = 0;   // first maximum, as tf.math.argmax
        float best = p.x;
        if (p.y > best) { best = p.y; am = 1; }
        if (p.z > best) { best = p.z; am = 2; }
        if (p.w > best) { best = p.w; am = 3; }
        cnt[0] += ((am == 0) ? 1.f : 0.f) == t.x;
        cnt[1] += ((am == 1) ? 1.f : 0.f) == t.y;
        cnt[2] += ((am == 2) ? 1.f : 0.f) == t.z;
        cnt[3] += ((am == 3) ? 1.f : 0.f) == t.w;
    }
    block_sum256(cnt, red);
    if (threadIdx.x == 0) {
        const float n = (float)a;
        out[img] = (((float)red[0][0] / n * cw.x + (float)red[1][0] / n * cw.y) + (float)red[2][0] / n * cw.z) + (float)red[3][0] / n * cw.w;
    }
}

// mean IoU of decoded predicted vs ground-truth boxes over the non-background anchors (metrics.py:76-171, including its
// conventions: widths clamped at 0, corners c -+ (w-1)/2, areas w*h, +1 in the intersection extents, epsilon in the
// denominator, 0/0 = NaN for an image without objects).  anchors: [a][4] = (cx, cy, w, h).  One block per image.
__global__ void __launch_bounds__(256) box_iou_kernel(const float* __restrict__ y_true, const float* __restrict__ y_pred,
                                                      const float* __restrict__ anchors, float4 sd, int a, float* __restrict__ out) {
    __shared__ float red[2][256];
    const int img = blockIdx.x;
    float s_iou = 0.f, s_nb = 0.f;
    for (int i = threadIdx.x; i < a; i += 256) {
        const float4 t = ld4(y_true + ((long long)img * a + i) * 4), p = ld4(y_pred + ((long long)img * a + i) * 4);
        const float4 an = ld4(anchors + (long long)i * 4);
        const float nb = (fabsf(t.x) + fabsf(t.y) + fabsf(t.z) + fabsf(t.w)) > 0.f ? 1.f : 0.f;
        float c[2][6];   // xmin, ymin, xmax, ymax, width, height of (pred, true)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 o = q == 0 ? p : t;
            const float cx = (o.x * sd.x * an.z + an.x) * nb, cy = (o.y * sd.y * an.w + an.y) * nb;
            const float wd = fmaxf(0.f, (expf(o.z * sd.z) - 1.f) * an.z) * nb, hg = fmaxf(0.f, (expf(o.w * sd.w) - 1.f) * an.w) * nb;
            c[q][0] = (cx - (wd - 1.f) / 2.f) * nb; c[q][1] = (cy - (hg - 1.f) / 2.f) * nb;
            c[q][2] = (cx + (wd - 1.f) / 2.f) * nb; c[q][3] = (cy + (hg - 1.f) / 2.f) * nb;
            c[q][4] = wd; c[q][5] = hg;
        }
        const float wi = fmaxf(0.f, fminf(c[1][2], c[0][2]) - fmaxf(c[1][0], c[0][0]) + 1.f) * nb;
        const float hi = fmaxf(0.f, fminf(c[1][3], c[0][3]) - fmaxf(c[1][1], c[0][1]) + 1.f) * nb;
        const float inter = wi * hi;
        s_iou += inter / (c[0][4] * c[0][5] + c[1][4] * c[1][5] - inter + KEPS);
        s_nb += nb;
    }
    const float sums[2] = {s_iou, s_nb};
    block_sum256(sums, red);
    if (threadIdx.x == 0) out[img] = red[0][0] / red[1][0];
}

}  // namespace

extern "C" {

int ssdseg_head_gather(ssdseg_ctx* ctx, const ssdseg_view* in, float* out, int b, int in_img_elems, int c, int out_off_elems,
                       int out_img_elems, int reverse) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(out != nullptr, 3);
    SSDSEG_ARG(b > 0, 4);
    SSDSEG_ARG(in_img_elems > 0 && in_img_elems % 4 == 0, 5);
    SSDSEG_ARG(c > 0 && c % 4 == 0 && in_img_elems % c == 0, 6);
    SSDSEG_ARG(out_off_elems >= 0 && out_off_elems % 4 == 0, 7);
    SSDSEG_ARG(out_img_elems >= out_off_elems + in_img_elems && out_img_elems % 4 == 0, 8);
    const long long total = (long long)b * (in_img_elems / 4);
    SSDSEG_LAUNCH(ctx, 8.0 * b * in_img_elems, 0.0, head_gather_kernel, dim3(ew_blocks(total)), dim3(256), 0, in->x, in->scale, in->shift,
                  in->act, out, b, in_img_elems, c, out_off_elems, out_img_elems, reverse);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_softmax_rows(ssdseg_ctx* ctx, const ssdseg_view* in, float* out, int rows, int c) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(in != nullptr && in->x != nullptr && ((in->scale == nullptr) == (in->shift == nullptr)), 2);
    SSDSEG_ARG(out != nullptr, 3);
    SSDSEG_ARG(rows > 0, 4);
    SSDSEG_ARG(c == 4, 5);
    SSDSEG_LAUNCH(ctx, 32.0 * rows, 0.0, softmax_rows4_kernel, dim3(ew_blocks(rows)), dim3(256), 0, in->x, in->scale, in->shift, in->act, out,
                  (long long)rows);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_metric_label_accuracy(ssdseg_ctx* ctx, const float* y_true, const float* y_pred, int b, int a, int c,
                                 const float* class_weights_host, float* out) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(y_true != nullptr, 2);
    SSDSEG_ARG(y_pred != nullptr, 3);
    SSDSEG_ARG(b > 0 && a > 0, 4);
    SSDSEG_ARG(c == 4, 6);
    SSDSEG_ARG(class_weights_host != nullptr, 7);
    SSDSEG_ARG(out != nullptr, 8);
    SSDSEG_LAUNCH(ctx, 32.0 * b * a, 0.0, label_accuracy_kernel, dim3(b), dim3(256), 0, y_true, y_pred, a,
                  f4_of(class_weights_host), out);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

int ssdseg_metric_box_iou(ssdseg_ctx* ctx, const float* y_true, const float* y_pred, const float* anchors_centroids, const float* stds4_host,
                          int b, int a, float* out) {
    SSDSEG_ARG(ctx != nullptr, 1);
    SSDSEG_ARG(y_true != nullptr, 2);
    SSDSEG_ARG(y_pred != nullptr, 3);
    SSDSEG_ARG(anchors_centroids != nullptr, 4);
    SSDSEG_ARG(stds4_host != nullptr, 5);
    SSDSEG_ARG(b > 0 && a > 0, 6);
    SSDSEG_ARG(out != nullptr, 8);
    SSDSEG_LAUNCH(ctx, 32.0 * b * a, 0.0, box_iou_kernel, dim3(b), dim3(256), 0, y_true, y_pred, anchors_centroids,
                  f4_of(stds4_host), a, out);
    SSDSEG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
