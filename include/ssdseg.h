/*
 * ssdseg.h -- C-ABI of libssdseg_hip.so: the MI355X (gfx950) hot path of `ssdseglib`.
 *
 * The reference (matteo-stat/multi-task-learning-object-detection-semantic-segmentation) is pure Python on
 * TensorFlow/Keras: it has no FFI of its own.  The boundary replaced here is therefore the set of TensorFlow
 * ops its hot path invokes; every entry point below cites the reference call
 * sites (file:line under the reference root) whose arithmetic it replaces.  The Python host
 * (`ssdseglib/_hip.py`, ctypes) is the only caller; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no C++/torch types.  All tensors are dense fp32, NHWC for activations,
 *     HWIO ([kh][kw][cin][cout]) for dense conv kernels, [kh][kw][c] for depthwise kernels, [cin][cout] for
 *     pointwise kernels (== Keras layouts, so get_weights()/set_weights() are memcpy).
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`.
 *   - every function returns 0 on success, -(hipError_t) for a HIP failure, or SSDSEG_EINVAL (-1000-n) for
 *     argument n being invalid.  Nothing throws across the boundary.  `ssdseg_last_error()` returns a
 *     thread-local description of the last failure.
 *   - launches are asynchronous on the ctx stream; `ssdseg_ctx_sync` waits.  A ctx is single-threaded.
 *   - kernels never allocate.  Scratch (BN partial sums, weight-gradient partial slabs, top-k histograms) comes
 *     from a ctx-owned workspace that grows on demand *outside* of launches (ssdseg_ctx_reserve).
 *
 * "Activation view" -- how conv + BatchNorm(train) + ReLU6 are fused:
 *   a conv kernel writes its RAW output y and per-block partial (sum, sum-of-squares) per channel; a tiny
 *   finalize kernel turns those into per-channel (scale, shift) = (gamma*invstd, beta - mean*gamma*invstd);
 *   every CONSUMER applies a = act(scale*y + shift) while loading.  So each activation is written once (raw)
 *   and never re-written normalised.  `ssdseg_view` describes such an input.
 *
 * "Gradient view" -- BatchNorm backward folded into the consumer of dY:
 *   given g = dL/d(act output), raw y and per-channel coefficients, the conv backward kernels form
 *       dy = scale * mask(z) * g + k1 * y + k0,   z = scale*y + shift,  mask = act'(z)
 *   on load (k1, k0 come from ssdseg_bn_bwd_finalize).  With scale == NULL the view is the identity (dy = g).
 */
#ifndef SSDSEG_H
#define SSDSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSDSEG_VERSION 1
#define SSDSEG_EINVAL(n) (-1000 - (n))

/* activation applied by a view (Keras ReLU(max_value=...) semantics) */
enum {
    SSDSEG_ACT_NONE = 0,  /* linear (MobileNetV2 project BN: models.py:110-111)                     */
    SSDSEG_ACT_RELU = 1,  /* tf.nn.relu, grad iff z > 0 (ShuffleNetV2 backbone: models.py:529,540)    */
    SSDSEG_ACT_RELU6 = 2, /* tf.nn.relu6, grad iff 0 < z < 6 (models.py:67,90; blocks.py:30,...)      */
    SSDSEG_ACT_ZERO = 3   /* ReLU(max_value=0.0): output 0, grad 0 (quirk Q1: blocks.py:4,76,134)     */
};

typedef struct ssdseg_ctx ssdseg_ctx;

/* input view: a = act(scale[c] * x + shift[c]); scale == NULL -> a = act(x) */
typedef struct {
    const float* x;
    const float* scale;
    const float* shift;
    int32_t act;
    int32_t _pad;
} ssdseg_view;

/* gradient view: dy = scale[c]*mask(scale[c]*y+shift[c])*g + k1[c]*y + k0[c]; scale == NULL -> dy = g */
typedef struct {
    const float* g;
    const float* y;
    const float* scale;
    const float* shift;
    const float* k1;
    const float* k0;
    int32_t act;
    int32_t _pad;
} ssdseg_gview;

/* ---------------------------------------------------------------- context, memory, timing */
const char* ssdseg_last_error(void);
int ssdseg_version(void);
int ssdseg_device_count(int* count_host);
/* stream == NULL: the ctx creates (and owns) a non-blocking stream; otherwise it borrows the caller's hipStream_t. */
int ssdseg_ctx_create(int device, void* stream, ssdseg_ctx** out_host);
int ssdseg_ctx_destroy(ssdseg_ctx* ctx);
int ssdseg_ctx_sync(ssdseg_ctx* ctx);
/* Weight-gradient kernels run on an internal side stream, concurrently with the rest of the backward pass.  Every entry point
 * that synchronises, copies, records an event, all-reduces or runs the optimizer joins it implicitly; a caller that hands the
 * gradient buffers to ANOTHER library on the ctx stream calls this first. */
int ssdseg_ctx_join(ssdseg_ctx* ctx);
/* on != 0: the launches that follow go to the side stream (after everything queued so far); on == 0: back to the ctx stream.
 * For callers that issue a weight-gradient entry point themselves (ssdseg_pwconv_bwd does this internally). */
int ssdseg_ctx_side(ssdseg_ctx* ctx, int on);
/* ssdseg_ctx_side_mark: remembers the current end of the side stream; ssdseg_ctx_side_wait_mark: the ctx stream waits for that point
 * -- and only for it: side-stream work queued after the mark keeps running beside the ctx stream (a join would wait for it too).
 * Used by the Python engine between the detection branch (side stream) and the layers that need its gradients. */
int ssdseg_ctx_side_mark(ssdseg_ctx* ctx);
int ssdseg_ctx_side_wait_mark(ssdseg_ctx* ctx);
/* enabled == 0: everything on the ctx stream from now on (used by bench.py to time a kernel without a co-running neighbour);
 * enabled != 0: side stream back on (if the ctx has one). */
int ssdseg_ctx_side_enable(ssdseg_ctx* ctx, int enabled);
/* Deferred column sums.  Weight-gradient kernels split their reduction over pixel ranges and leave partial slabs that a
 * fixed-order column sum folds into dW; nothing reads dW before the optimizer (Keras `train_step`: gradients are consumed by
 * `optimizer.apply_gradients`, NB03#cell16), so with enabled != 0 those ~80 small launches per backward pass are recorded
 * instead of launched and go out as ONE launch at the next join (ssdseg_ctx_join, and every entry point that joins: sync, copies,
 * all-reduce, Adam).  Same summation order either way: gradients are bit-identical with deferral on or off.
 * enabled == 0 flushes what is pending and returns to one launch per column sum (the engine's backward pass ends that way, so an
 * entry point called after it folds its own slabs).  Calls that keep deferral on without a join fold what is pending once the
 * slab arena reaches SSDSEG_COLSUM_ARENA_MB (default 4096) instead of growing it further. */
int ssdseg_colsum_defer(ssdseg_ctx* ctx, int enabled);
int ssdseg_ctx_reserve(ssdseg_ctx* ctx, size_t workspace_bytes);
int ssdseg_ctx_device_name(ssdseg_ctx* ctx, char* buf_host, size_t buf_len);
/* Debug poison (off by default; tests only).  While on != 0: ssdseg_malloc fills every new allocation with the 32-bit word
 * 0x7FF0DEAD (a NaN as fp32) and returns after the fill has finished; every workspace and deferred-colsum arena handout is filled
 * with the same word on the ctx stream before the caller's kernels run.  handouts (may be NULL): number of poisoned workspace /
 * arena handouts since the ctx was created. */
int ssdseg_ctx_debug_poison(ssdseg_ctx* ctx, int on, long long* handouts);
int ssdseg_malloc(ssdseg_ctx* ctx, size_t bytes, void** out_host);
int ssdseg_free(ssdseg_ctx* ctx, void* ptr);
int ssdseg_memcpy_h2d(ssdseg_ctx* ctx, void* dst, const void* src_host, size_t bytes);
int ssdseg_memcpy_d2h(ssdseg_ctx* ctx, void* dst_host, const void* src, size_t bytes);
int ssdseg_memcpy_d2d(ssdseg_ctx* ctx, void* dst, const void* src, size_t bytes);
int ssdseg_memset(ssdseg_ctx* ctx, void* dst, int value, size_t bytes);
/* HIP events on the ctx stream (bench.py times kernels with these, not with torch events) */
int ssdseg_event_create(ssdseg_ctx* ctx, void** out_host);
int ssdseg_event_destroy(ssdseg_ctx* ctx, void* ev);
int ssdseg_event_record(ssdseg_ctx* ctx, void* ev);
int ssdseg_event_elapsed_ms(ssdseg_ctx* ctx, void* ev_start, void* ev_stop, float* ms_host);
/* Per-kernel timing: while enabled, every kernel launch of this library is bracketed by HIP events on the ctx
 * stream and aggregated per kernel symbol together with the launch's ALGORITHMIC bytes / flops.
 * report: one "kernel\tcount\ttotal_ms\tbytes\tflops\n" line per kernel into buf_host. */
int ssdseg_timing_enable(ssdseg_ctx* ctx, int enable);
int ssdseg_timing_reset(ssdseg_ctx* ctx);
/* bracket only launches of one kernel symbol (low overhead inside a timed region); NULL or "" = every kernel */
int ssdseg_timing_filter(ssdseg_ctx* ctx, const char* kernel);
int ssdseg_timing_report(ssdseg_ctx* ctx, char* buf_host, size_t buf_len);
/* Overlapped uploads (new: the reference feeds tf.data batches, NB03#cell8,16).  Pinned host memory and a copy stream
 * per ctx: ssdseg_upload_async enqueues host -> device on the copy stream; ssdseg_upload_fence marks a point on the ctx stream
 * (typically right after the kernels / copies that read a staging buffer) and after_fence != 0 keeps an upload behind the last
 * such point -- but not behind work queued after it, which is what lets the upload of batch i+1 run under step i;
 * ssdseg_upload_join makes the ctx stream wait for the uploads queued so far; ssdseg_upload_sync blocks the host until they are
 * done (before the pinned source is overwritten). */
int ssdseg_host_alloc(ssdseg_ctx* ctx, size_t bytes, void** out_host);
int ssdseg_host_free(ssdseg_ctx* ctx, void* ptr_host);
int ssdseg_upload_fence(ssdseg_ctx* ctx);
/* src_host: pinned (ssdseg_host_alloc: the call returns at once) or ordinary pageable memory (the call returns when the
 * runtime has staged it; the transfer still overlaps the kernels of the ctx stream) */
int ssdseg_upload_async(ssdseg_ctx* ctx, void* dst, const void* src_host, size_t bytes, int after_fence);
int ssdseg_upload_join(ssdseg_ctx* ctx);
int ssdseg_upload_sync(ssdseg_ctx* ctx);

/* ---------------------------------------------------------------- data parallelism (new: SURVEY.md 8(e))
 * The reference has no distributed code (single-process Keras fit, NB03#cell16); the boundary replaced is what
 * tf.distribute.MirroredStrategy would do around NB03#cell14-16: per-replica BatchNormalization statistics and mining pool
 * (losses.py:74-75,113,127), ONE sum-all-reduce of the gradients per step.  One process per GPU; RCCL over xGMI (librccl.so is
 * dlopen'ed at the first call below).  Rank 0 obtains a 128-byte id and hands it to the other ranks by any host-side means
 * (ssdseglib/_parallel.py: a file next to MASTER_PORT); every rank then calls ssdseg_comm_init_rank -- a collective call.
 * (SURVEY.md 8(b2) sketched `ssdseg_comm_init_all`, the single-process / all-devices form; the bench contract is one process
 * per GPU, hence init_rank.) */
#define SSDSEG_COMM_ID_BYTES 128
enum { SSDSEG_COMM_F32 = 0, SSDSEG_COMM_F64 = 1 };
enum { SSDSEG_COMM_SUM = 0, SSDSEG_COMM_MAX = 1 };
int ssdseg_comm_unique_id(void* id_host, size_t id_bytes);
int ssdseg_comm_init_rank(ssdseg_ctx* ctx, const void* id_host, size_t id_bytes, int rank, int world);
int ssdseg_comm_destroy(ssdseg_ctx* ctx);
int ssdseg_comm_info(ssdseg_ctx* ctx, int* rank_host, int* world_host);
/* The step's one collective, stream-ordered behind the backward pass (joins the weight-gradient side stream first):
 * grads[count] <- sum over ranks (ssdseg_adam_step's grad_scale = 1/world makes it the mean);
 * state[state_count] <- MEAN over ranks (BatchNormalization moving_mean / moving_variance, models.py:66,89,111: every replica
 * updates them from its own shard, the average keeps replicas and checkpoints identical).  Either may be NULL / 0. */
int ssdseg_allreduce_grads(ssdseg_ctx* ctx, float* grads, size_t count, float* state, size_t state_count);
/* in-place all-reduce of a small device buffer (timing max over ranks, barriers) and broadcast from `root` */
int ssdseg_allreduce(ssdseg_ctx* ctx, void* buf, size_t count, int dtype, int op);
int ssdseg_broadcast(ssdseg_ctx* ctx, float* buf, size_t count, int root);

/* ---------------------------------------------------------------- K1+K2: stem conv
 * Conv2D 3x3 stride 2 SAME on the rescaled image, tiny Cin (models.py:187 Rescaling x/127.5-1, :196 -> :65;
 * ShuffleNetV2 stem models.py:622,628 with bias).  in = x*in_scale + in_offset fused into the load.
 * y: [n][ho][wo][cout] raw.  stats: [nparts][2][cout] partial (sum, sumsq), may be NULL.
 * ssdseg_stem_conv_parts() tells how many partial rows the launch writes. */
int ssdseg_stem_conv_parts(int n, int h, int w, int cout, int* nparts_host);
int ssdseg_stem_conv_fwd(ssdseg_ctx* ctx, const float* x, const float* w, const float* bias, float* y,
                         int n, int h, int wdt, int cin, int cout, float in_scale, float in_offset,
                         float* stats);
/* dW (and dbias) only: the image needs no gradient.  dw: [3][3][cin][cout]. */
int ssdseg_stem_conv_bwd_weight(ssdseg_ctx* ctx, const float* x, const ssdseg_gview* dy, float* dw,
                                float* dbias, int n, int h, int wdt, int cin, int cout, float in_scale,
                                float in_offset);

/* ---------------------------------------------------------------- K3+K4: depthwise 3x3 (stride 1|2, dilation >= 1)
 * DepthwiseConv2D / depthwise half of SeparableConv2D, SAME padding, depth multiplier 1
 * (models.py:88,236,242,524,533,542,577,586; blocks.py:33,38,43,122,152).
 * TF SAME: out = ceil(in/s), pad_total = max((out-1)*s + (k-1)*d + 1 - in, 0), before = pad_total/2. */
int ssdseg_dwconv_parts(int n, int h, int w, int c, int stride, int dilation, int* nparts_host);
int ssdseg_dwconv_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, const float* w, float* y, int n, int h, int wdt,
                      int c, int stride, int dilation, float* stats);
/* dx (= dL/d(act output of the producer), same shape as the input) and dw [3][3][c] in one pass.
 * accumulate != 0: dx += result (fan-out taps).  dx may be NULL (only dw wanted). */
int ssdseg_dwconv_bwd(ssdseg_ctx* ctx, const ssdseg_view* in, const float* w, const ssdseg_gview* dy, float* dx,
                      float* dw, int n, int h, int wdt, int c, int stride, int dilation, int accumulate);
/* The same plus the BatchNormalization backward of the layer that FEEDS this conv (in = act(scale*x + shift) is a BN view,
 * models.py:66-67 -> :88): the kernel that writes dx also reduces sum(mask*dx) and sum(mask*dx*xhat) over it, so the
 * 6x-wide expand tensors are not re-read by ssdseg_bn_bwd_reduce.  Valid when this conv is the only consumer of the BN
 * output (accumulate = 0) or the LAST of several to contribute (accumulate != 0: dx already holds the other consumers'
 * gradients -- a backbone tap that also feeds the heads -- and the sums are taken over the completed dx).
 * Outputs (dgamma, dbeta may be NULL): as ssdseg_bn_bwd_reduce. */
int ssdseg_dwconv_bwd_bn(ssdseg_ctx* ctx, const ssdseg_view* in, const float* w, const ssdseg_gview* dy, float* dx,
                         float* dw, int n, int h, int wdt, int c, int stride, int dilation, int accumulate,
                         const float* in_mean, const float* in_invstd, float* in_dgamma, float* in_dbeta, float* in_k1,
                         float* in_k0);

/* ---------------------------------------------------------------- K5: pointwise 1x1 conv == GEMM [m,k] x [k,n]
 * Conv2D 1x1 / pointwise half of SeparableConv2D (models.py:65,110,527,...; blocks.py:28,58,70,109).
 * fp32-input MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products, fp32 accumulate.
 * ldx/ldy: row strides in floats (>= k / >= n) so a layer can read/write a channel slice of a concat buffer
 * (K10: Concatenate is a write offset, never a copy). */
int ssdseg_pwconv_parts(int m, int n, int* nparts_host);
int ssdseg_pwconv_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int ldy, int m,
                      int k, int n, float* stats);
/* The tile GEMM behind the forward streams the weights with the reduction channel contiguous (Wt[n][k]); ssdseg_pwconv_fwd
 * makes that copy itself, one small launch per call.  A caller that owns all layers of a model (ssdseglib/_engine.py) does it
 * ONCE per step for all of them instead: ssdseg_pwconv_wt_floats() tells whether the default dispatch of a shape uses such a
 * copy (k*n floats, 0 = no), ssdseg_transpose_batch() fills the copies of a whole table of layers in one launch (table on the
 * device: per matrix four 64-bit words {source pointer W[k][n], destination pointer Wt[n][k], k, n}; max_tiles = the largest
 * ceil(k/32)*ceil(n/32) of the table; total_floats = sum of k*n, for the timing registry), and ssdseg_pwconv_fwd_wt() takes the
 * copy (wt may be NULL = as ssdseg_pwconv_fwd; a copy passed for a shape that runs on another kernel family is ignored). */
int ssdseg_pwconv_wt_floats(int m, int ldx, int k, int n, int* floats_host);
int ssdseg_transpose_batch(ssdseg_ctx* ctx, const long long* table, int nmat, int max_tiles, long long total_floats);
int ssdseg_pwconv_fwd_wt(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, const float* wt, float* y, int ldy,
                         int m, int k, int n, float* stats);
/* dx[m][k] = dy[m][n] * w^T; residual != NULL: dx += residual (Add backward, models.py:162);
 * accumulate != 0: dx += previous contents. */
int ssdseg_pwconv_bwd_data(ssdseg_ctx* ctx, const ssdseg_gview* dy, int ldy, const float* w, float* dx, int ldx,
                           int m, int k, int n, const float* residual, int ldr, int accumulate);
/* dw[k][n] = sum_m in[m][k] * dy[m][n] */
int ssdseg_pwconv_bwd_weight(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy,
                             float* dw, int m, int k, int n);
/* Both of the above in one call.  For k <= 32 and n <= 192 (the MBConv expand convs, models.py:65 with 6x expansion) ONE
 * kernel produces dx and dw from a single pass over the gradient view; other shapes run the two kernels above.
 * (dy->y is, in every use the host package makes of this entry point, the convolution's own raw forward output.) */
int ssdseg_pwconv_bwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy, const float* w,
                      float* dx, int lddx, float* dw, int m, int k, int n, const float* residual, int ldr,
                      int accumulate);
/* dx + dw plus the BatchNormalization backward of the layer that FEEDS this conv (in is that BN's view, models.py:89-90 ->
 * :110): the backward-data kernel's float4 epilogue reduces sum(mask*dx) and sum(mask*dx*xhat) while it stores dx.  Only
 * valid when this conv is the ONLY consumer of the BN output.  Outputs as ssdseg_bn_bwd_reduce (dgamma, dbeta may be NULL).
 * lddx is a multiple of 4; a dx or an input that is not 16-byte aligned runs the plain GEMM and ssdseg_bn_bwd_reduce. */
int ssdseg_pwconv_bwd_bn(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, int ldy, const float* w,
                         float* dx, int lddx, float* dw, int m, int k, int n, const float* in_mean,
                         const float* in_invstd, float* in_dgamma, float* in_dbeta, float* in_k1, float* in_k0);

/* ---------------------------------------------------------------- K6: dense 3x3 stride 1 SAME (implicit GEMM)
 * Conv2D 3x3 in the DeepLabV3+ decoder (blocks.py:117,127).  w: [3][3][cin][cout]. */
int ssdseg_conv3x3_parts(int n, int h, int w, int cin, int cout, int* nparts_host);
int ssdseg_conv3x3_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int n, int h,
                       int wdt, int cin, int cout, float* stats);
/* Large layers (the DeepLabV3+ decoder conv) run in the Winograd form, whose weight gradient wants the ACTIVATED input act(scale*x+shift)
 * in a zero-bordered copy [n][h+2][w+2][cin].  ssdseg_conv3x3_saved_floats reports that copy's size for a shape (0: the shape does
 * not use it -- call the plain entry points); ssdseg_conv3x3_fwd_saved writes it (one pass; the forward kernel then reads IT, with
 * the identity view) and ssdseg_conv3x3_bwd_weight_saved consumes it, so the view is applied once per step instead of twice.
 * Same results as ssdseg_conv3x3_fwd / _bwd_weight (dy: the materialised gradient, i.e. an identity gradient view). */
int ssdseg_conv3x3_saved_floats(int n, int h, int w, int cin, int cout, long long* floats_host);
int ssdseg_conv3x3_fwd_saved(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int n, int h, int wdt, int cin,
                             int cout, float* stats, float* xsaved);
/* the same when the channels [0, c_from) of xsaved already hold the activated input (ssdseg_bilinear_fwd_padded wrote them over
 * a border that was zero when the buffer was made): only channels [c_from, cin) of `in` are viewed and copied. */
int ssdseg_conv3x3_fwd_saved_from(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const float* w, float* y, int n, int h,
                                  int wdt, int cin, int cout, float* stats, float* xsaved, int c_from);
int ssdseg_conv3x3_bwd_weight_saved(ssdseg_ctx* ctx, const float* xsaved, const float* dy, float* dw, int n, int h, int wdt, int cin,
                                    int cout);
int ssdseg_conv3x3_bwd_data(ssdseg_ctx* ctx, const ssdseg_gview* dy, const float* w, float* dx, int ldx, int n,
                            int h, int wdt, int cin, int cout, int accumulate);
/* The same plus the BatchNormalization backward of the layer that FEEDS this conv (in = that BN's view of the conv input; the
 * decoder's 256 -> output_channels conv behind sepconv-batchnorm, blocks.py:121-126): for the narrow, tap-expanded form the sums
 * sum(mask*dx), sum(mask*dx*xhat) ride in the epilogue of the GEMM that writes dx; other shapes run ssdseg_conv3x3_bwd_data
 * followed by ssdseg_bn_bwd_reduce.  Only valid when this conv is the ONLY consumer of the BN output (dx is overwritten).
 * Outputs as ssdseg_bn_bwd_reduce (dgamma, dbeta may be NULL). */
int ssdseg_conv3x3_bwd_data_bn(ssdseg_ctx* ctx, const ssdseg_view* in, const ssdseg_gview* dy, const float* w, float* dx, int ldx,
                               int n, int h, int wdt, int cin, int cout, const float* in_mean, const float* in_invstd,
                               float* in_dgamma, float* in_dbeta, float* in_k1, float* in_k0);
int ssdseg_conv3x3_bwd_weight(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_gview* dy, float* dw,
                              int n, int h, int wdt, int cin, int cout);

/* dy->g <- scale*mask(scale*y+shift)*g + k1*y + k0 in place: materialises a BatchNorm-backward gradient view ONCE for a consumer
 * that would otherwise re-form it many times (the dense 3x3 conv reads every dy element 9x in backward-data and again in the
 * weight gradient).  Afterwards the consumer uses the identity gradient view {dy->g}. */
int ssdseg_gview_materialize(ssdseg_ctx* ctx, const ssdseg_gview* dy, int ld, int m, int c);

/* ---------------------------------------------------------------- K7/K8: BatchNormalization (training) + activation
 * Keras BatchNormalization defaults eps 1e-3, momentum 0.99 (models.py:66,89,111,...; blocks.py:29,...).
 * finalize: partial (sum, sumsq)[nparts][2][c] over `count` samples per channel ->
 *   mean, biased var -> scale = gamma*rsqrt(var+eps), shift = beta - mean*scale, invstd;
 *   moving_mean <- mom*mm + (1-mom)*mean; moving_var <- mom*mv + (1-mom)*var*count/(count-1) (Bessel, App. B.3).
 *   The fold is float64; var is clamped at 0 (float32 partial sums of a constant channel can fold to slightly less), and
 *   count == 1 (the GAP branch at batch 1) feeds the biased var to moving_var: no 0/0 factor.  moving_* may be NULL in training.
 * training == 0: scale/shift from the moving statistics (inference), partials ignored. */
int ssdseg_bn_finalize(ssdseg_ctx* ctx, const float* stats, int nparts, int c, double count, const float* gamma,
                       const float* beta, float eps, float momentum, float* moving_mean, float* moving_var,
                       float* mean, float* invstd, float* scale, float* shift, int training);
/* plain per-channel (sum, sumsq) of a tensor [m][c] (row stride ld) -> stats[nparts][2][c] (for tensors
 * not produced by one of the conv kernels, e.g. the GAP branch) */
int ssdseg_channel_stats_parts(int m, int c, int* nparts_host);
int ssdseg_channel_stats(ssdseg_ctx* ctx, const float* x, int ld, int m, int c, float* stats);
/* materialise out = view(in) (+ view(residual)): Add (models.py:162,593), taps, concat slices; residual may be NULL */
int ssdseg_bn_apply(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, const ssdseg_view* residual, int ldr, float* out,
                    int ldo, int m, int c);
/* BN backward reductions: dbeta = sum mask*g, dgamma = sum mask*g*xhat over [m][c]; writes
 * dgamma, dbeta (each BatchNormalization has one use, so they are stored, not accumulated) and the gview
 * coefficients k1, k0. */
int ssdseg_bn_bwd_reduce(ssdseg_ctx* ctx, const float* g, int ldg, const float* y, int ldy, int m, int c,
                         const float* scale, const float* shift, const float* mean, const float* invstd, int act,
                         float* dgamma, float* dbeta, float* k1, float* k0);
/* dst (+)= src over [m][c] with row strides (gradient fan-in: Concatenate / Add backward) */
int ssdseg_axpby(ssdseg_ctx* ctx, const float* src, int lds, float* dst, int ldd, int m, int c, float a, float b);

/* ---------------------------------------------------------------- K11: GlobalAveragePooling2D keepdims (blocks.py:57) */
int ssdseg_gap_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, float* out, int n, int hw, int c);
/* dx[n][hw][c] (+)= g[n][c] / hw */
int ssdseg_gap_bwd(ssdseg_ctx* ctx, const float* g, float* dx, int n, int hw, int c, int accumulate);

/* ---------------------------------------------------------------- K12: UpSampling2D bilinear, half-pixel (blocks.py:61,104,129)
 * out[n][h*fy][w*fx][c] written with row stride ldo (concat slice). */
int ssdseg_bilinear_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, float* out, int ldo, int n, int h, int wdt,
                        int c, int fy, int fx);
int ssdseg_bilinear_bwd(ssdseg_ctx* ctx, const float* g, int ldg, float* dx, int ldx, int n, int h, int wdt, int c,
                        int fy, int fx, int accumulate);
/* the forward written into the INTERIOR of a bordered tensor out[n][h*fy + 2][wdt*fx + 2][ldo] (border untouched): the x4
 * up-sampled ASPP output (blocks.py:104) lands directly in the zero-bordered input copy the decoder's 3x3 conv kernels read
 * (blocks.py:117; ssdseg_conv3x3_fwd_saved_from), instead of in a plain concat buffer that a padding pass copies again. */
int ssdseg_bilinear_fwd_padded(ssdseg_ctx* ctx, const ssdseg_view* in, int ldx, float* out, int ldo, int n, int h, int wdt,
                               int c, int fy, int fx);

/* ---------------------------------------------------------------- K12+K13: mask head tail
 * logits [n][h][w][c] --x(fy,fx) bilinear--> softmax -> probabilities (output-mask, blocks.py:128-130),
 * optionally fused with the weighted cross-entropy (losses.py:294-303): loss[n] = -sum_c w_c sum_px y*log(clip p).
 * prob may be NULL (training does not need it stored); y_true/loss may be NULL (inference).  n <= 65535 (the image is a grid
 * dimension of the forward kernels; the same holds for ssdseg_mask_head_fwd_dice and ssdseg_mask_head_fwd_bootstrap).
 * The clip interval is [lo, hi] in float32: lo = float(1e-7), hi = 1.f - float(1e-7) = 1 - 2^-23 (NOT 1 - 1e-7, which float32
 * does not have).  The loss takes log(min(max(p, lo), hi)).  The gradient follows the clip: a labelled (pixel, class) entry whose
 * probability is outside [lo, hi] contributes a zero dL/dp, so a pixel whose labelled probabilities are all outside has an
 * exactly zero row of d loss / d logits; inside, dL/dp_c = -w_c y_c / p_c. */
int ssdseg_mask_head_fwd(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                         const float* y_true, const float* class_weights_host, float* prob, float* loss);
/* dlogits (low resolution) = upsample^T( softmax'( dL/dp ) ), dL/dp = -loss_scale * w_c * y / p inside the clip */
int ssdseg_mask_head_bwd(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                         const float* y_true, const float* class_weights_host, float loss_scale, float* dlogits);
/* The same head trained with the reference's dice / dice_square losses (losses.py:175-264; squared != 0: dice_square).  The
 * forward also leaves, per image, the eight coefficients the backward needs (coef [n][8]: A_c = -2 w_c / (T_c + eps),
 * B_c = w_c (2 I_c + eps) / (T_c + eps)^2 with I_c = sum y p, T_c = sum (y + p) [sum (y^2 + p^2)] over the image's pixels), so
 * that dL/dp_c = A_c y_c + B_c [2 p_c] is formed per pixel in the backward kernels exactly like the cross-entropy's.
 * prob, loss may be NULL (not both loss and coef). */
int ssdseg_mask_head_fwd_dice(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                              const float* y_true, const float* class_weights_host, int squared, float* prob, float* loss,
                              float* coef);
int ssdseg_mask_head_bwd_dice(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                              const float* y_true, const float* coef, int squared, float loss_scale, float* dlogits);
/* The same head trained with the bootstrapped cross-entropy (hard-pixel mining; not in the reference).  Per image, with
 * l_i = -sum_c w_c y_ic log(clip p_ic) the cross-entropy term of pixel i (float32, the expression ssdseg_mask_head_fwd sums):
 * thresh = the keep-th largest l of the image (1 <= keep <= H*W, H*W = h*fy * wdt*fx), found by an exact radix select;
 * pixel i is kept when l_i >= thresh -- EVERY pixel tied with the keep-th value, so kept[img] may exceed keep (no tie-break by
 * index); loss[img] = sum of the kept l.  keep = H*W is the cross-entropy.  The forward writes pixel_loss [n][H*W] (4 bytes per
 * pixel) and thresh [n]; the backward reads both back and compares the STORED l with thresh, so its keep decision is the
 * forward's bit for bit: dlogits = upsample^T(softmax'(dL/dp)) with the cross-entropy's dL/dp for kept pixels and an exact zero
 * row for dropped ones.  prob, kept, loss may be NULL. */
int ssdseg_mask_head_fwd_bootstrap(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                                   const float* y_true, const float* class_weights_host, int keep, float* prob,
                                   float* pixel_loss, float* thresh, int* kept, float* loss);
int ssdseg_mask_head_bwd_bootstrap(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                                   const float* y_true, const float* class_weights_host, const float* pixel_loss,
                                   const float* thresh, float loss_scale, float* dlogits);
/* the same loss from given probabilities (API surface: losses.bootstrapped_cross_entropy called directly): y_true, p [n][hw][c],
 * loss [n] */
int ssdseg_bootstrap_ce_loss(ssdseg_ctx* ctx, const float* y_true, const float* p, int n, int hw, int c,
                             const float* class_weights_host, int keep, float* loss);
/* Void pixels.  A pixel is LABELLED iff any component of its y_true row is non-zero, otherwise VOID (a class index >= 4 of a
 * mask file, the fill_class = 255 padding of a crop or a mosaic: an all-zero one-hot row).  The cross-entropy entries above
 * ignore a void pixel as they stand (zero term, zero gradient).  The _void entries below are their dice and bootstrapped twins,
 * argument for argument, with void pixels left out; without a void pixel every output equals the twin's bit for bit.
 *   dice / dice_square: T_c sums over the labelled pixels only (I_c has no void term anyway), loss and coef are formed from I, T
 *   as before, and dL/dp of a void pixel is an exact zero row (its dz is +0).  An image without a labelled pixel has loss 0.
 *   bootstrapped: keep [n] (int32, written) = min(L, max(1, ceil(keep_fraction L))) in double from L = the image's labelled
 *   pixels, counted on the device (0 for L = 0; 0 < keep_fraction <= 1); thresh = the keep-th largest LABELLED l (+inf for
 *   L = 0); a void pixel is never kept nor counted in kept and its gradient row is zero: its stored pixel_loss is -1, below
 *   every thresh.  No host synchronisation.  prob, kept, loss may be NULL. */
int ssdseg_mask_head_fwd_dice_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                                   const float* y_true, const float* class_weights_host, int squared, float* prob, float* loss,
                                   float* coef);
int ssdseg_mask_head_bwd_dice_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                                   const float* y_true, const float* coef, int squared, float loss_scale, float* dlogits);
int ssdseg_mask_head_fwd_bootstrap_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                                        const float* y_true, const float* class_weights_host, double keep_fraction, float* prob,
                                        float* pixel_loss, float* thresh, int* keep, int* kept, float* loss);
int ssdseg_mask_head_bwd_bootstrap_void(ssdseg_ctx* ctx, const float* logits, int n, int h, int wdt, int c, int fy, int fx,
                                        const float* y_true, const float* class_weights_host, const float* pixel_loss,
                                        const float* thresh, float loss_scale, float* dlogits);
int ssdseg_bootstrap_ce_loss_void(ssdseg_ctx* ctx, const float* y_true, const float* p, int n, int hw, int c,
                                  const float* class_weights_host, double keep_fraction, float* loss);
/* SSD head plumbing: Reshape(-1, 4) + Concatenate(axis=1) (blocks.py:155; models.py:256,271).  Forward: the activated
 * head tensor of one feature map, in[b][in_img_elems] (channel of element r = r % c), is written to
 * out[b][out_off_elems + r] of a buffer with out_img_elems floats per image.  reverse != 0 copies the other way
 * (gradient of the concat back to the head; `in->x` is then the concat-side buffer, `out` the head-side one). */
int ssdseg_head_gather(ssdseg_ctx* ctx, const ssdseg_view* in, float* out, int b, int in_img_elems, int c,
                       int out_off_elems, int out_img_elems, int reverse);

/* ---------------------------------------------------------------- K13..K15: detection losses
 * softmax over the class axis of head logits (models.py:259) */
int ssdseg_softmax_rows(ssdseg_ctx* ctx, const ssdseg_view* in, float* out, int rows, int c);
/* confidence_loss (losses.py:52-172) + localization_loss (losses.py:5-49) forward and gradient in one call.
 * y_labels/p_labels: [b][a][c] (p = probabilities); y_boxes/p_boxes: [b][a][4].
 * conf_loss/loc_loss: [b].  d_logits: dL/d(pre-softmax logits) [b][a][c], d_boxes: dL/d p_boxes, both already
 * scaled by loss_scale (= loss_weight / batch for Keras' SUM_OVER_BATCH_SIZE).  Either may be NULL.
 * keep_mask (optional, uint8 [b*a]) receives the hard-negative selection (1 = kept background anchor). */
int ssdseg_det_loss(ssdseg_ctx* ctx, const float* y_labels, const float* p_labels, const float* y_boxes,
                    const float* p_boxes, int b, int a, int c, float loss_scale, float* conf_loss, float* loc_loss,
                    float* d_logits, float* d_boxes, uint8_t* keep_mask);
/* ssdseg_det_loss with a weight of its own per output: d_logits is scaled by conf_scale, d_boxes by loc_scale (compile's
 * loss_weights may differ between 'output-labels' and 'output-boxes').  ssdseg_det_loss is this call with both scales equal. */
int ssdseg_det_loss_scaled(ssdseg_ctx* ctx, const float* y_labels, const float* p_labels, const float* y_boxes,
                           const float* p_boxes, int b, int a, int c, float conf_scale, float loc_scale, float* conf_loss,
                           float* loc_loss, float* d_logits, float* d_boxes, uint8_t* keep_mask);
/* Focal confidence loss (not in the reference) + localization_loss, forward and gradient in one call.  With ph = clip(p, eps,
 * 1 - eps), eps = 1e-7 (the clip of confidence_loss):
 *   per anchor  FL = -sum_c alpha_c y_c (1 - ph_c)^gamma log ph_c
 *   per image   conf_loss[i] = sum over ALL anchors of FL / max(#non-background anchors of image i, 1)
 * No hard-negative mining: every anchor contributes, background included, and no image depends on another one.
 *   dFL/dp_c = g_c = -alpha_c y_c inside(p_c) [ (1 - ph_c)^gamma / ph_c - gamma (1 - ph_c)^(gamma - 1) log ph_c ]
 *   d_logits_j = conf_scale / max(npos_i, 1) * p_j (g_j - sum_k p_k g_k)
 * inside(p) = 1 for eps <= p <= 1 - eps, else 0 (the gradient of the clip).  gamma = 0, alpha = 1 is the softmax cross-entropy
 * over every anchor; the gamma term is then exactly 0.  alpha4_host: four finite weights >= 0; gamma finite, >= 0.
 * loc_loss and d_boxes (scaled by loc_scale) are bit-identical to ssdseg_det_loss's.  Any of the four outputs may be NULL. */
int ssdseg_det_loss_focal(ssdseg_ctx* ctx, const float* y_labels, const float* p_labels, const float* y_boxes,
                          const float* p_boxes, int b, int a, int c, const float* alpha4_host, float gamma, float conf_scale,
                          float loc_scale, float* conf_loss, float* loc_loss, float* d_logits, float* d_boxes);
/* IoU-family box regression loss (not in the reference), forward and gradient: the DETR-style sum
 *   loss[n] = sum_i box_i (smooth_l1_weight * sl1_i + term_i) / max(sum_i box_i, 1)
 * over the anchors i of image n.  box_i = 1 if |t.x| + |t.y| + |t.z| + |t.w| > 0 for the target offsets t (localization_loss's
 * test), sl1_i is localization_loss's smooth-L1 of t - p, and term_i compares the DECODED target box g and predicted box p.
 * Both offsets o decode alike against the default box (ax, ay, aw, ah) = anchors_centroids[i] (device, [a][4]) and the stds s:
 *   cx = o.x s.x aw + ax, cy = o.y s.y ah + ay, w = max((exp(o.z s.z) - 1) aw, 0), h = max((exp(o.w s.w) - 1) ah, 0),
 *   corners cx -+ w/2, cy -+ h/2: continuous boxes, without the +1 / (w - 1)/2 pixel conventions of ssdseg_metric_box_iou and
 *   ssdseg_decode_boxes.
 *   iw = max(min(px1, gx1) - max(px0, gx0), 0), ih likewise, I = iw ih, U = pw ph + gw gh - I, IoU = I / (U + 1e-7),
 *   ew = max(px1, gx1) - min(px0, gx0), eh likewise
 *   kind 0 (IoU):  term = 1 - IoU
 *   kind 1 (GIoU): term = 1 - IoU + (E - U) / (E + 1e-7), E = ew eh
 *   kind 2 (DIoU): term = 1 - IoU + ((pcx - gcx)^2 + (pcy - gcy)^2) / (ew^2 + eh^2 + 1e-7)
 * d_boxes = loc_scale * d loss[n] / d p through the decode, written for EVERY anchor (exact zeros where box = 0).  At a clamp
 * (w, h, iw, ih at 0) the derivative is 0; at a tie of a min / max it follows the strict comparison of the spec
 * (tests/_iou_loss_oracle.py).  An untrained head decodes to boxes of size 0, where the overlap terms alone have a zero gradient
 * on the size offsets of most anchors: smooth_l1_weight (finite, >= 0; 0 allowed) keeps the smooth-L1 term next to them.
 * stds4_host: four finite values > 0.  loc_loss [b] and d_boxes [b][a][4] may each be NULL.  Finite inputs only.  Three launches
 * (per-block partials, per-image fold in fixed order, gradient), no float atomics. */
int ssdseg_loc_loss_iou(ssdseg_ctx* ctx, const float* y_boxes, const float* p_boxes, const float* anchors_centroids,
                        const float* stds4_host, int b, int a, int kind, float smooth_l1_weight, float loc_scale,
                        float* loc_loss, float* d_boxes);
/* exact top-k selection used by the mining step (tf.math.top_k semantics: larger value first, lower index
 * first among equals, losses.py:131): mask[i] = 1 for the k selected entries of values[n]. */
int ssdseg_topk_mask(ssdseg_ctx* ctx, const float* values, int n, int k, uint8_t* mask);
/* dice / dice_square (losses.py:175-264), API surface only: loss[n] from y_true, p [n][hw][c]; n <= 65535 */
int ssdseg_dice_loss(ssdseg_ctx* ctx, const float* y_true, const float* p, int n, int hw, int c,
                     const float* class_weights_host, int squared, float* loss);
/* the same with void pixels (all-zero y_true rows) left out of T_c, as ssdseg_mask_head_fwd_dice_void; squared 0 or 1 */
int ssdseg_dice_loss_void(ssdseg_ctx* ctx, const float* y_true, const float* p, int n, int hw, int c,
                          const float* class_weights_host, int squared, float* loss);

/* ---------------------------------------------------------------- K16: anchor matching + offset encoding
 * DataEncoderDecoder._encode_ground_truth_labels_boxes (datacoder.py:205-300).
 * anchors_corners [a][4] (xmin,ymin,xmax,ymax); gt [b][gmax][5] (label,xmin,ymin,xmax,ymax), gt_count [b].
 * labels [b][a][c] one-hot, boxes [b][a][4] offsets; match (optional) [b][a] int32 matched gt index or -1. */
int ssdseg_encode_targets(ssdseg_ctx* ctx, const float* anchors_corners, int a, const float* gt,
                          const int32_t* gt_count, int b, int gmax, int c, float iou_threshold, const float* stds4_host,
                          float* labels, float* boxes, int32_t* match);

/* ---------------------------------------------------------------- compact batch -> engine buffers
 * DataEncoderDecoder.read_and_encode (datacoder.py:302-347) on the device: the host uploads what the files hold -- uint8 pixels
 * [b][h][w][3], uint8 class indices [b][h][w], ground-truth rows -- and these two calls (+ ssdseg_encode_targets) produce the
 * float32 image (tf.cast :327), the float32 one-hot mask [b][h][w][c] (tf.one_hot :332: an index >= c gives an all-zero row) and
 * the mirrored ground truth of the samples whose flip[n] != 0 (tf.image.flip_left_right :341-342; boxes xmin' = W - xmax,
 * xmax' = W - xmin :202-203, quirk Q8).  images_u8 or mask_index_u8 may be NULL (only the other is expanded); flip may be NULL.
 * One image holds fewer than 2^31 bytes (h * w * 3 < 2^31, else the argument error for h): in-image offsets are 32-bit, as in
 * ssdseg_rgb_augment, ssdseg_gather_inputs and ssdseg_crop_inputs; any b (launches of at most 65,535 samples). */
int ssdseg_expand_inputs(ssdseg_ctx* ctx, const uint8_t* images_u8, const uint8_t* mask_index_u8, const uint8_t* flip, float* images_f32,
                         float* mask_onehot, int b, int h, int w, int c);
/* gt [b][gmax][5] = (label, xmin, ymin, xmax, ymax), in place, rows g < gt_count[n] of the samples with flip[n] != 0 */
int ssdseg_flip_gt_boxes(ssdseg_ctx* ctx, float* gt, const int32_t* gt_count, const uint8_t* flip, int b, int gmax, float image_width);
/* DataEncoderDecoder.augmentation_rgb_channels (datacoder.py:434-466) on the compact pixels, as the host spec
 * datacoder._augment_rgb: hue shift, saturation scale, contrast about the per-(image, channel) mean of the hue- and
 * saturation-adjusted image, brightness shift (the [0, 1]-scale deltas on 0..255 values, quirk Q11), clip to [0, 255].
 * draws4_host = (hue_delta, saturation_factor, contrast_factor, brightness_delta): ONE set for the whole batch, as
 * tf.image.random_* draw one scalar per call on a 4-D tensor.  images_u8 [b][h][w][3]; flip [b] or NULL (mirror the
 * flagged images left-right, as ssdseg_expand_inputs does); means [b][3] (device, out); images_f32 [b][h][w][3] (out).
 * The means are reduced in a fixed order (block partials in the ctx workspace): the result is the same bits on every run. */
int ssdseg_rgb_augment(ssdseg_ctx* ctx, const uint8_t* images_u8, const uint8_t* flip, const float* draws4_host,
                       float* means, float* images_f32, int b, int h, int w);
/* Device-resident training set (datacoder.ResidentDataset): the reference's NB03#cell8 chain -- shuffle(len), map(read_and_encode),
 * batch, map(augmentation_rgb_channels) -- with the samples kept in HBM as the files hold them.  A batch is a list of pool sample
 * indices and flip flags, both HOST arrays ([b] int32 / [b] uint8 or NULL) that are validated here (every index in [0, n_pool),
 * else the argument error and nothing is launched) and passed to the kernels by value: no copy, no synchronisation, and the
 * caller may overwrite them as soon as the call returns.
 * ssdseg_gather_inputs: pool_images u8 [n_pool][h][w][3], pool_masks u8 [n_pool][h][w]; output sample n is pool sample
 *   index_host[n], mirrored where flip_host[n] != 0: images_f32 [b][h][w][3] and mask_onehot [b][h][w][c] hold the bits
 *   ssdseg_expand_inputs (datacoder.py:302-347) writes for the same samples stacked on the host -- or, with draws4_host != NULL,
 *   the image and means [b][3] (device, out) the bits of ssdseg_rgb_augment (datacoder.py:434-466; same fixed reduction order).
 *   Either pool / destination pair may be NULL; draws need the image pair and means.  Pool offsets are 64-bit.
 * ssdseg_gather_gt: pool_gt [n_pool][gmax][5], pool_cnt [n_pool] -> gt [b][gmax][5], gt_count [b]; rows g < count of a flagged
 *   sample mirrored as ssdseg_flip_gt_boxes does (xmin' = W - xmax, xmax' = W - xmin), rows past the count written as zeros. */
int ssdseg_gather_inputs(ssdseg_ctx* ctx, const uint8_t* pool_images, const uint8_t* pool_masks, int n_pool, const int32_t* index_host,
                         const uint8_t* flip_host, const float* draws4_host, float* means, float* images_f32, float* mask_onehot, int b, int h,
                         int w, int c);
int ssdseg_gather_gt(ssdseg_ctx* ctx, const float* pool_gt, const int32_t* pool_cnt, int n_pool, const int32_t* index_host,
                     const uint8_t* flip_host, float* gt, int32_t* gt_count, int b, int gmax, float image_width);

/* Random crop / zoom-out augmentation on the device (datacoder.random_crop_windows; the reference has none: opt-in), the step in
 * front of the flip and the colour augmentation.  windows_host [b][4] float32 = (x0, y0, w, h) per output sample, in source-pixel
 * units (pixel i covers [i, i + 1)); a window may reach outside the image (zoom-out) and the output has the sample's own size.
 * The source is a pool and a HOST index list ([b] int32, every index in [0, n_src)) or, with index_host == NULL, a plain batch
 * (output n from source n; b <= n_src).  Indices, windows and fill are validated here and passed to the kernels by value, as in
 * ssdseg_gather_inputs: no copy, no synchronisation, the caller may overwrite them as soon as the call returns.  Every window
 * must be finite with 1 <= w <= 16 W, 1 <= h <= 16 H, |x0| <= 16 W, |y0| <= 16 H (else the argument error, nothing is launched).
 * All arithmetic is float32 in the order of the host spec datacoder._crop_resample / _crop_gt, without FMA contraction: the
 * results are its bytes.  The outputs are a dense compact batch for ssdseg_expand_inputs / ssdseg_rgb_augment /
 * ssdseg_flip_gt_boxes / ssdseg_encode_targets and must not overlap the sources.
 * ssdseg_crop_inputs: src_images u8 [n_src][h][w][3] -> images_u8 [b][h][w][3], bilinear: with sx = w / W, X = (x0 + (ox + 0.5)
 *   sx) - 0.5, xf = floor(X), ax = X - xf (Y, yf, ay likewise), v = top + (bot - top) ay of top = t00 + (t01 - t00) ax and bot
 *   = t10 + (t11 - t10) ax, byte = floor(v + 0.5); a tap outside the image is fill_rgb_host[3] (NULL: 0, 0, 0).  src_masks u8
 *   [n_src][h][w] -> mask_index_u8 [b][h][w], nearest: source pixel (floor(y0 + (oy + 0.5) sy), floor(x0 + (ox + 0.5) sx)),
 *   fill_class (0..255) outside.  Either source / destination pair may be NULL.  A window (0, 0, W, H) copies the sample.
 *   Pool offsets are 64-bit; h * w * 3 < 2^31.  flip_host [b] u8 or NULL: the batch's flip flags, which the crop does NOT apply
 *   but writes to flip_out [b] (device, 0 / 1) as they are -- the `flip` argument of the calls that follow, delivered in the
 *   kernel arguments like the other host lists (a resident batch has no upload to carry them).
 * ssdseg_crop_gt: src_gt [n_src][gmax][5] = (label, xmin, ymin, xmax, ymax), src_cnt [n_src] -> gt [b][gmax][5], gt_count [b]:
 *   a row is kept iff its centre ((xmin + xmax) / 2, (ymin + ymax) / 2) has x0 <= cx < x0 + w and y0 <= cy < y0 + h, and after
 *   x' = (x - x0) (W / w), y' = (y - y0) (H / h) and the clip to [0, W] / [0, H] both xmax' - xmin' >= 1 and ymax' - ymin' >= 1.
 *   Kept rows stay in their order (ssdseg_encode_targets is order-sensitive), rows past the new count are zeros, the count may
 *   be 0.  A window exactly (0, 0, W, H) copies the sample's rows verbatim (no centre test, no clip). */
int ssdseg_crop_inputs(ssdseg_ctx* ctx, const uint8_t* src_images, const uint8_t* src_masks, int n_src, const int32_t* index_host,
                       const float* windows_host, const uint8_t* fill_rgb_host, int fill_class, const uint8_t* flip_host, uint8_t* flip_out,
                       uint8_t* images_u8, uint8_t* mask_index_u8, int b, int h, int w);
int ssdseg_crop_gt(ssdseg_ctx* ctx, const float* src_gt, const int32_t* src_cnt, int n_src, const int32_t* index_host,
                   const float* windows_host, float* gt, int32_t* gt_count, int b, int gmax, int h, int w);

/* Mosaic augmentation on the device (datacoder.random_mosaic; the reference has none: opt-in), in the crop's place in front of the
 * flip and the colour augmentation; a batch is cropped or assembled, not both.  Output sample n of size H x W is cut by the split
 * point split_host[n] = (px, py), 0 <= px <= W, 0 <= py <= H, into the quadrants k = 0 top-left [0, px) x [0, py), 1 top-right
 * [px, W) x [0, py), 2 bottom-left [0, px) x [py, H), 3 bottom-right [px, W) x [py, H); a quadrant of zero width or height is empty
 * and contributes nothing.  Tile k shows the window windows_host[n][k] = (x0, y0, w, h), in source-pixel units, of source sample
 * index4_host[n][k], mapped onto quadrant k = (qx, qy, qw, qh).  All three lists are HOST arrays ([b][4] int32, [b][2] int32,
 * [b][4][4] float32, none may be NULL), validated here -- every index in [0, n_src), every split inside the image, every window,
 * those of empty quadrants included, finite with 1 <= w <= 16 W, 1 <= h <= 16 H, |x0| <= 16 W, |y0| <= 16 H, else the argument
 * error and nothing is launched -- and passed to the kernels by value, 16 samples per launch: no copy, no synchronisation, the
 * caller may overwrite them as soon as the call returns.  All arithmetic is float32 in the order of the host spec
 * datacoder._mosaic_resample / _mosaic_gt, without FMA contraction; the divisions w / qw, qw / w, ... are done on the host: the
 * results are the spec's bytes.  The outputs are a dense compact batch, as those of the crop calls, and must not overlap the sources.
 * ssdseg_mosaic_inputs: output pixel (ox, oy) of quadrant k has the source coordinate u = x0 + ((ox - qx) + 0.5) (w / qw), v
 *   likewise; the byte is ssdseg_crop_inputs' bilinear value of the four taps around (u, v) in source index4_host[n][k] (a tap
 *   outside the source IMAGE -- not the window -- is fill_rgb_host[3], NULL: 0, 0, 0), the class index its nearest pixel
 *   (fill_class, 0..255, outside).  Either source / destination pair may be NULL.  A sample with split (W, H) and tile-0 window
 *   (0, 0, W, H) is a copy of its source.  flip_host [b] u8 or NULL: the batch's flags, not applied but written to flip_out [b]
 *   (device, 0 / 1), as ssdseg_crop_inputs does.  Pool offsets are 64-bit; h * w * 3 < 2^31.
 * ssdseg_mosaic_gt: src_gt [n_src][gmax][5] = (label, xmin, ymin, xmax, ymax), src_cnt [n_src] -> gt [b][gmax][5], gt_count [b].
 *   Tiles are visited in the order 0..3, empty quadrants skipped, the source's rows in their order.  A row is kept iff its centre
 *   has x0 <= cx < x0 + w and y0 <= cy < y0 + h and, after x' = qx + (x - x0) (qw / w) clipped to [qx, qx + qw] and y' likewise,
 *   both extents are >= 1.  Kept rows are concatenated in visiting order; the first gmax are written, gt_count = min(total, gmax),
 *   rows past the count are zeros.  A tile whose quadrant is the whole image and whose window is exactly (0, 0, W, H) copies its
 *   source's rows verbatim (no centre test, no clip). */
int ssdseg_mosaic_inputs(ssdseg_ctx* ctx, const uint8_t* src_images, const uint8_t* src_masks, int n_src, const int32_t* index4_host,
                         const int32_t* split_host, const float* windows_host, const uint8_t* fill_rgb_host, int fill_class,
                         const uint8_t* flip_host, uint8_t* flip_out, uint8_t* images_u8, uint8_t* mask_index_u8, int b, int h, int w);
int ssdseg_mosaic_gt(ssdseg_ctx* ctx, const float* src_gt, const int32_t* src_cnt, int n_src, const int32_t* index4_host,
                     const int32_t* split_host, const float* windows_host, float* gt, int32_t* gt_count, int b, int gmax, int h, int w);

/* ---------------------------------------------------------------- training metrics
 * Per-image values of the three metric factories NB03#cell14 passes to compile(metrics=...); Keras averages them.
 * jaccard_iou_segmentation_masks_metric (metrics.py:35-47): SOFT Jaccard, inter = sum t*p, total = sum(t+p) over pixels,
 *   sum_c w_c * inter_c / (total_c - inter_c + 1e-7).  from_logits = 1: src = the low-resolution logits [n][h][w][4], p =
 *   softmax(bilinear x(fy,fx)) recomputed per pixel (the training step never stores output-mask); from_logits = 0:
 *   src = probabilities [n][h][w][4], fy = fx = 1.  y_true [n][h*fy][w*fx][4].  out [n].  n <= 65535. */
int ssdseg_metric_mask_iou(ssdseg_ctx* ctx, const float* src, int n, int h, int wdt, int c, int fy, int fx, int from_logits,
                           const float* y_true, const float* class_weights_host, float* out);
/* the same metric with total = sum (t + p) over the LABELLED pixels only (a pixel whose y_true row is all zero is void) */
int ssdseg_metric_mask_iou_void(ssdseg_ctx* ctx, const float* src, int n, int h, int wdt, int c, int fy, int fx, int from_logits,
                                const float* y_true, const float* class_weights_host, float* out);
/* categorical_accuracy_metric (metrics.py:204-216): per class #anchors with one_hot(argmax p)[c] == y_true[c], / a,
 *   weighted sum over classes.  y_true, y_pred [b][a][4]; out [b]. */
int ssdseg_metric_label_accuracy(ssdseg_ctx* ctx, const float* y_true, const float* y_pred, int b, int a, int c,
                                 const float* class_weights_host, float* out);
/* jaccard_iou_bounding_boxes_metric (metrics.py:76-171): offsets decoded against the default boxes (anchors_centroids
 *   [a][4] = cx, cy, w, h; device), IoU with the reference's conventions, averaged over the non-background anchors of
 *   y_true (NaN for an image without objects, like the reference).  y_true, y_pred [b][a][4]; out [b]. */
int ssdseg_metric_box_iou(ssdseg_ctx* ctx, const float* y_true, const float* y_pred, const float* anchors_centroids,
                          const float* stds4_host, int b, int a, float* out);

/* ---------------------------------------------------------------- K17..K19: inference tail
 * DecodeBoxesCentroidsOffsets.call (layers.py:58-79): offsets [b][a][4] -> corners (ymin,xmin,ymax,xmax) */
int ssdseg_decode_boxes(ssdseg_ctx* ctx, const float* offsets, const float* anchors_centroids, int b, int a,
                        const float* stds4_host, float* corners);
/* NonMaximumSuppression.call (layers.py:141-162) == tf.image.combined_non_max_suppression semantics
 * (App. B.9) + repack: out [b][max_total][6] = (label, prob, xmin, ymin, xmax, ymax), zero padded;
 * valid [b] = number of real detections. */
int ssdseg_combined_nms(ssdseg_ctx* ctx, const float* corners, const float* probs, int b, int a, int c,
                        int max_per_class, int max_total, float iou_threshold, float score_threshold, float* out,
                        int32_t* valid);
/* ssdseg_combined_nms with Gaussian Soft-NMS score decay (Bodla et al. 2017; the soft_nms_sigma of
 * tf.image.non_max_suppression_with_scores, per class as above; TF's combined NMS has no soft form).  Same layouts and argument
 * checks; soft_nms_sigma must be finite and > 0 (off is ssdseg_combined_nms itself).  Per image and class, every class competing:
 *   1. s_i = probs[i][cls]; a candidate is alive iff s_i > score_threshold.
 *   2. at most max_per_class times: pick the alive k with the largest CURRENT s (ties: lowest anchor), record (s_k, k, cls) with
 *      the decayed score and kill k; for every alive i, iou = the hard kernel's IoU (raw corners, no +1, a degenerate box overlaps
 *      nothing): iou > iou_threshold kills i, otherwise s_i = s_i * w and i dies if s_i <= score_threshold.
 *   3. w = float32(exp(-0.5 * x * x / float64(soft_nms_sigma))), x = float64(iou), evaluated in double in that order: the
 *      correctly rounded float32 weight on any host with an IEEE double exp, so a host restatement (layers.soft_nms_reference)
 *      agrees bit for bit; iou == 0 gives w == 1 exactly.
 *   4. merge as above: (decayed score desc, anchor asc, class asc), max_total rows (label, decayed score, xmin, ymin, xmax, ymax).
 * iou_threshold = 1 is the pure Gaussian Soft-NMS (Bodla's sigma = 2 * soft_nms_sigma); a sigma so large that every w rounds to
 * 1 (1e30) gives the bytes of ssdseg_combined_nms.  No atomics, no host synchronisation: the same bytes on every run. */
int ssdseg_combined_nms_soft(ssdseg_ctx* ctx, const float* corners, const float* probs, int b, int a, int c,
                             int max_per_class, int max_total, float iou_threshold, float score_threshold,
                             float soft_nms_sigma, float* out, int32_t* valid);
/* SegmentationSuppression.call (layers.py:203-210): class-present flags over the WHOLE batch (quirk Q6) */
int ssdseg_seg_suppress(ssdseg_ctx* ctx, const float* mask_prob, int n_pixels_total, int c, const float* probs,
                        int rows, float* probs_out);

/* ---------------------------------------------------------------- test-set evaluation (NB03#cell21-29) on the engine's outputs
 * jaccard_iou_semantic_segmentation (evaluators.py:189-247) per image and class, without the one-hot mask: prob [n][hw][c] is the
 *   `output-mask` buffer as the inference engine leaves it, mask_index_u8 [n][hw] the class indices of a compact / resident
 *   batch; y = (index == class) (an index >= c is an all-zero one-hot pixel, tf.one_hot, as ssdseg_expand_inputs), I = sum y*p,
 *   T = sum (y + p), iou_out [n][c] = I / (T - I + 1e-7) (evaluators.py:236-241; the mean over the samples is the caller's).
 *   1 <= c <= 8.  Block partials in the ctx workspace, added in index order in double: the same bits on every run. */
int ssdseg_eval_mask_jaccard(ssdseg_ctx* ctx, const float* prob, const uint8_t* mask_index_u8, int n, int hw, int c, float* iou_out);
/* The same pass with the segmentation protocol's two options; the probabilities are read once for all three outputs.
 *   ignore_void != 0: T sums over the labelled pixels only (index < c); a void pixel (index >= c) then enters neither I nor T.
 *   confusion_out [n][c][c] (int32, rows true, columns predicted): for every labelled pixel of true class k,
 *   confusion[k][argmax_j p_j] += 1, the lowest index among equal probabilities (np.argmax); void pixels enter no row, whatever
 *   ignore_void says.  void_out [n]: the image's pixels with an index >= c.  Integer counts, folded in a fixed order.
 *   iou_out, confusion_out and void_out may each be NULL (not all three).  With ignore_void == 0 iou_out holds the bits of
 *   ssdseg_eval_mask_jaccard.  n <= 65535, hw < 2^28, 1 <= c <= 8. */
int ssdseg_eval_mask_scores(ssdseg_ctx* ctx, const float* prob, const uint8_t* mask_index_u8, int n, int hw, int c, int ignore_void,
                            float* iou_out, int32_t* confusion_out, int32_t* void_out);
/* The IoU step of average_precision_object_detection (evaluators.py:6-62 inside :65-186): det [n][r][6] = (label, confidence,
 *   xmin, ymin, xmax, ymax) as ssdseg_combined_nms writes it, gt [n][gmax][5] = (label, xmin, ymin, xmax, ymax) and gt_count [n]
 *   as ssdseg_gather_gt / the compact loader hold them; best_out [n][r] = the largest IoU of the prediction with a ground-truth
 *   box OF THE SAME LABEL -- pixel-inclusive extents (+1), 1e-7 in the denominator, float32, no FMA contraction -- and 0 when the
 *   image has no ground truth, no label matches, or the prediction's label is 0 (background / an empty NMS row).  The IoU, not a
 *   true-positive flag: the caller thresholds it once per AP threshold. */
int ssdseg_eval_det_best_iou(ssdseg_ctx* ctx, const float* det, const float* gt, const int32_t* gt_count, int n, int r, int gmax,
                             float* best_out);

/* ---------------------------------------------------------------- K20: Adam (Keras 2.13, NB03#cell14)
 * m += (g-m)(1-b1); v += (g^2-v)(1-b2); p -= lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps), one flat bucket.
 * grad_scale multiplies g first (1/world_size after the RCCL sum). */
int ssdseg_adam_step(ssdseg_ctx* ctx, float* params, const float* grads, float* m, float* v, size_t count,
                     float lr, float beta1, float beta2, float eps, int step, float grad_scale);

/* ---------------------------------------------------------------- K20b: SGD and AdamW with a weight-decay run table
 * Decoupled weight decay as Keras 2.13's optimizers apply it (`weight_decay`): p1 = p - (lr * lambda) * p before the update, with
 * lr the learning rate itself (for AdamW: not the bias-corrected alpha).  WHERE it applies is a run table over the flat bucket:
 *   run_end   [nruns] device, ascending exclusive end offsets in elements; run r covers [run_end[r-1], run_end[r]), run 0 from 0
 *   run_decay [nruns] device, the coefficient lambda of each run
 * Elements at or beyond the last run_end take lambda = 0, and so does every element when nruns == 0 (both pointers NULL then).
 * Boundaries are arbitrary (ShuffleNetV2's 58- / 122-channel vectors put them at offsets = 2 mod 4: the four lanes of one
 * float4 may belong to different runs).  A run with lambda == 0 leaves p1 = p bit for bit.  The table is read through the
 * caches, a few entries per block (csrc/decay_runs.h): no per-element mask stream.  Whatever the table holds -- ends that do
 * not ascend, ends beyond `count` -- the kernels touch nothing outside [0, count) of the buffers and nothing outside the
 * table's nruns entries (the decay then lands where the table's own order says, which is the caller's business).
 * nruns is at most SSDSEG_DECAY_RUNS_MAX (a 48 KiB table, far beyond the few hundred runs of the models here); more is an
 * argument error.
 *
 * ssdseg_sgd_step -- Keras 2.13 SGD, g' = g * grad_scale:
 *   momentum == 0:  p = p1 - lr g'                       (velocity may be NULL, it is not touched; 12 B per element)
 *   momentum  > 0:  v = momentum v - lr g';  p = p1 + v  (20 B per element)
 *        nesterov:  v likewise;  p = p1 + (momentum v - lr g')
 *   momentum in [0, 1); nesterov != 0 needs momentum > 0 to mean anything (with momentum == 0 it is ignored).
 * ssdseg_adamw_step -- ssdseg_adam_step applied to p1: the same kernel body with the decay compiled in; with nruns == 0 it IS
 *   ssdseg_adam_step's launch, bit for bit. */
#define SSDSEG_DECAY_RUNS_MAX 4096
int ssdseg_sgd_step(ssdseg_ctx* ctx, float* params, const float* grads, float* velocity, size_t count, float lr,
                    float momentum, int nesterov, float grad_scale, const long long* run_end, const float* run_decay,
                    int nruns);
int ssdseg_adamw_step(ssdseg_ctx* ctx, float* params, const float* grads, float* m, float* v, size_t count, float lr,
                      float beta1, float beta2, float eps, int step, float grad_scale, const long long* run_end,
                      const float* run_decay, int nruns);

/* ---------------------------------------------------------------- K20c: gradient clipping and the EMA of the weights
 * Keras 2.13's `global_clipnorm` (tf.clip_by_global_norm), `clipvalue` (tf.clip_by_value) and `use_ema`, on the device: the clip
 * factor depends on this step's gradients, so it is produced into device memory and consumed from there -- no download, no stall.
 *
 * ssdseg_grad_norm writes two floats:
 *   out[0] = |grad_scale| * sqrt(sum g_i^2)                     the global norm of the scaled gradient, rounded once to float
 *   out[1] = norm > clip_norm ? clip_norm / norm : 1            computed in double, rounded once
 * out[1] is exactly 1.0f when clip_norm <= 0 or not finite, for an all-zero bucket (no 0/0), for count == 0, and for a NaN norm
 * (the comparison fails; non-finite gradients then reach the weights as they do without clipping -- no step is skipped).
 * Squares and sums are fp64 (the square of a float is exact in double: no overflow at 1e30, no underflow at 1e-30).  `partials`
 * is scratch of ssdseg_grad_norm_parts(count) doubles -- a function of count alone, as the partition of the bucket is -- and the
 * reduction has one fixed order: two launches (blocks write partials, one block folds them), no atomics.  The same bucket gives
 * the same 8 bytes on every call and on every rank.  The entry joins the side stream first, like the step entries.
 *
 * ssdseg_sgd_step_clipped / ssdseg_adamw_step_clipped are ssdseg_sgd_step / ssdseg_adamw_step with
 *   g' = clampv((g * grad_scale) * s),  clampv(x) = x < -c ? -c : (x > c ? c : x)    (NaN passes through, as tf.clip_by_value)
 * in place of g' = g * grad_scale; everything after g' is the same element function.  s = *clip_scale (device, one float; NULL: 1),
 * c = clip_value (> 0; +inf: none; 0, negative or NaN is an argument error).  With *clip_scale == 1 and clip_value == +inf the
 * result is the unclipped entry's, bit for bit: for SGD at any grad_scale, for AdamW wherever g * grad_scale is exact (a
 * power-of-two grad_scale) -- the unclipped kernel fuses that product into m's update, elsewhere m differs by its one rounding.
 *
 * ssdseg_ema_update: ema += (p - ema) * (1 - momentum), 1 - momentum formed once in float; momentum in [0, 1].  ema == p is a
 * fixed point.  A 12 B per element pass of its own: it follows any of the three step entries. */
int ssdseg_grad_norm_parts(size_t count);
int ssdseg_grad_norm(ssdseg_ctx* ctx, const float* grads, size_t count, float grad_scale, float clip_norm, double* partials,
                     float* out);
int ssdseg_sgd_step_clipped(ssdseg_ctx* ctx, float* params, const float* grads, float* velocity, size_t count, float lr,
                            float momentum, int nesterov, float grad_scale, const long long* run_end, const float* run_decay,
                            int nruns, const float* clip_scale, float clip_value);
int ssdseg_adamw_step_clipped(ssdseg_ctx* ctx, float* params, const float* grads, float* m, float* v, size_t count, float lr,
                              float beta1, float beta2, float eps, int step, float grad_scale, const long long* run_end,
                              const float* run_decay, int nruns, const float* clip_scale, float clip_value);
int ssdseg_ema_update(ssdseg_ctx* ctx, float* ema, const float* params, size_t count, float momentum);

/* ---------------------------------------------------------------- K21: ShuffleNetV2-only ops
 * MaxPooling2D 3x3 stride 2 SAME (models.py:629); argmax-free backward (recomputes the window max). */
int ssdseg_maxpool3x3s2_fwd(ssdseg_ctx* ctx, const ssdseg_view* in, float* out, int n, int h, int wdt, int c);
int ssdseg_maxpool3x3s2_bwd(ssdseg_ctx* ctx, const ssdseg_view* in, const float* g, float* dx, int n, int h, int wdt,
                            int c);
/* channel shuffle (groups) of a concat of two halves: out[.., j*g + i] = view(in)[.., i*(c/g) + j]  (models.py:497-503);
 * the input is a view, so the lazily fused BatchNorm + ReLU of the concatenated branches is applied in the same pass.
 * inverse != 0 applies the inverse permutation (gradient path; pass an identity view). */
int ssdseg_channel_shuffle(ssdseg_ctx* ctx, const ssdseg_view* in, int ldi, float* out, int ldo, int m, int c, int groups,
                           int inverse);
/* General channel re-indexing: out[m][j] = table[j] >= 0 ? view(in)[m][table[j]] : 0 (+ previous contents when accumulate).
 * ShuffleNetV2 '1x' / '2x' split their stage-2 tensors into 58 / 122 channels; inside those units the branch tensors are
 * zero-padded to multiples of 4 and Split (models.py:573), the channel shuffle (models.py:497-503) and their gradients are
 * table lookups between the packed and the padded layouts.  table: device int32 [c_out]. */
int ssdseg_channel_gather(ssdseg_ctx* ctx, const ssdseg_view* in, int ldi, float* out, int ldo, long long m, int c_out,
                          const int32_t* table, int accumulate);
/* rows x cols block copy between row-major matrices of different leading dimension: parameters between their exact Keras
 * shapes (flat bucket) and the zero-padded shapes of those units; rows * cols < 2^31 - 2^21 */
int ssdseg_copy2d(ssdseg_ctx* ctx, float* dst, int ldd, const float* src, int lds, int rows, int cols);
/* The same for a table of blocks in ONE launch.  `table` (device): ncopies rows of six 64-bit words {dst pointer, ldd, src pointer,
 * lds, rows, cols}; max_elems = the largest rows * cols of the table (sizes the grid; < 2^31 - 4096), total_floats = their sum
 * (timing registry).
 * ShuffleNetV2 '1x' / '2x' (reference models.py:557-603: stage-2 branches of 58 / 122 channels) keep zero-padded copies of ~50
 * weight tensors: refreshing them and folding their gradients back was 160 launches of ~6 us per step. */
int ssdseg_copy2d_batch(ssdseg_ctx* ctx, const long long* table, int ncopies, int max_elems, long long total_floats);
/* g *= act'(x) in place: backward of a ReLU that follows an Add (ShuffleNetV2 basic unit, models.py:593-595) */
int ssdseg_act_bwd(ssdseg_ctx* ctx, float* g, int ldg, const float* x, int ldx, int m, int c, int act);

#ifdef __cplusplus
}
#endif
#endif /* SSDSEG_H */
