/* libunetdc_hip.so -- C ABI of the MI355X (gfx950) U-Net / U-Net-DC forward+backward kernels.
 *
 * This is the drop-in boundary for the hot path of malani86/unet-DC-segmentation.  The reference
 * has no FFI of its own: its boundary is the nn.Module contract of UNetDC / UNet plus autograd
 * (SURVEY.md section 8b), and every operator below replaces the ATen call the reference makes at
 * the cited line of /root/reference.  Conventions:
 *
 *   - plain C: raw DEVICE pointers, explicit sizes/strides, a hipStream_t passed as void*;
 *     no torch types, no C++ exceptions.  Every function returns 0 on success, a negative
 *     UNETDC_E* code otherwise; unetdc_last_error() returns a thread-local message.
 *   - the library never allocates or frees device memory: activations, packed weights and
 *     workspaces are owned by the caller (PyTorch's caching allocator in the Python host layer).
 *   - activations are NHWC ("pixel-major") in the compute type `dtype` (UNETDC_F32 / UNETDC_BF16):
 *     element (n,y,x,c) at ((n*H + y)*W + x)*ld + c.  `ld` (in elements, multiple of 16 bytes)
 *     lets a tensor be a channel slice of a wider buffer, which is how torch.cat
 *     (models/model_2.py:68,71,74,77) costs zero bytes: the up-convolution writes channels
 *     [0,C) and the encoder skip writes channels [C,2C) of one [pixels][2C] buffer.
 *   - the network input (NCHW fp32, train_DC_focal.py:250) and output (NCHW fp32 probabilities,
 *     model_2.py:80) keep the reference's layout; parameters and their gradients are fp32 in
 *     PyTorch layout (Conv2d [Cout][Cin][3][3], ConvTranspose2d [Cin][Cout][2][2]).
 *   - kernels are enqueued on the given stream and are re-entrant; reductions are two-stage with
 *     a fixed order (no float atomics), so results are bitwise reproducible.
 */
#ifndef UNETDC_HIP_H
#define UNETDC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNETDC_ABI_VERSION 2

#define UNETDC_F32 0
#define UNETDC_BF16 1

#define UNETDC_OK 0
#define UNETDC_EINVAL (-1)      /* bad argument (shape, alignment, null pointer) */
#define UNETDC_ELAUNCH (-2)     /* HIP reported an error for a launch */
#define UNETDC_EWORKSPACE (-3)  /* caller-provided workspace too small */

typedef void* unetdc_stream_t; /* hipStream_t */

int unetdc_version(void);
const char* unetdc_last_error(void);
/* symbol (as rocprofv3 prints it) of the matrix-core kernel the last conv/convT/wgrad call dispatched;
 * the library picks the kernel per layer shape, profiling tools use this to attribute time. */
const char* unetdc_last_kernel(void);

/* ---- weight packing (derived caches of the fp32 parameters; redo after optimizer.step()) ------
 * conv3x3:  w [Cout][Cin][3][3] -> w_fwd [9][Cout][Cin], w_dgrad [9][Cin][Cout] (taps flipped)
 * convT2x2: w [Cin][Cout][2][2] -> w_fwd [4*Cout][Cin] (row (a*2+b)*Cout+co), w_dgrad [4][Cin][Cout]
 * w_dgrad may be NULL (inference). */
int unetdc_pack_conv3x3(const float* w, void* w_fwd, void* w_dgrad, int cout, int cin, int dtype, unetdc_stream_t s);
int unetdc_pack_convT2x2(const float* w, void* w_fwd, void* w_dgrad, int cin, int cout, int dtype, unetdc_stream_t s);
/* Every layer in ONE launch (LDS-tiled transpose).  `table_dev` is a DEVICE array of n descriptors
 * sorted by `begin` = running sum of 32x32 channel tiles ((a/32)*(b/32) per tensor; a, b multiples
 * of 32); kind 0 = conv3x3 with (a,b) = (cout,cin), kind 1 = convT2x2 with (a,b) = (cin,cout);
 * `total_tiles` = the grand total.  Same images as the two calls above. */
typedef struct unetdc_pack_desc {
  const float* w;
  void* w_fwd;
  void* w_dgrad; /* nullable */
  int64_t begin;
  int32_t a, b;
  int32_t kind;
  int32_t pad;
} unetdc_pack_desc;
int unetdc_pack_many(const unetdc_pack_desc* table_dev, int n, int64_t total_tiles, int dtype, unetdc_stream_t s);

/* ---- optimizer step ---------------------------------------------------------------------------
 * Replaces `optimizer.step()` of torch.optim.Adam (/root/reference/train_DC_focal.py:224,255; train.py:125) AND the
 * re-pack above, in one launch: for every parameter   g <- grad_scale * g;   m <- m + (1-beta1)(g - m);
 * v <- beta2 v + (1-beta2) g g;   p <- p - lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)
 * (torch's _fused_adam_ formulation; no weight decay / amsgrad, which the reference does not use), and the packed
 * images of the conv / convT weights are rewritten from the NEW p.
 * `table_dev`: DEVICE array of n descriptors sorted by `begin` (first workgroup of the tensor); a packed tensor takes
 * (a/32)*(b/32) workgroups, a plain one ceil(numel/4096); `total_blocks` = the grand total.  The gradient of tensor i is
 * flat_grad[g_off .. g_off + numel): the flat fp32 buffer the backward kernels write (parameters() order).
 * wf / wd may be NULL for a packed-kind tensor (then only p, m, v are updated).  `step` counts from 1. */
typedef struct unetdc_adam_desc {
  float* p; float* m; float* v;   /* fp32 master parameter, exp_avg, exp_avg_sq (same layout as p) */
  void* wf; void* wd;             /* packed images in `dtype`, or NULL */
  int64_t g_off, begin, numel;
  int32_t a, b;                   /* kind 0: (cout, cin); kind 1: (cin, cout); kind 2: unused */
  int32_t kind;                   /* 0 conv3x3 (packed), 1 convT2x2 (packed), 2 plain */
  int32_t flags;                  /* bit 0: weight decay applies (unetdc_adam_step_ex; unetdc_adam_step ignores the word) */
} unetdc_adam_desc;
int unetdc_adam_step(const unetdc_adam_desc* table_dev, int n, int64_t total_blocks, const float* flat_grad, double lr,
                     double beta1, double beta2, double eps, int64_t step, double grad_scale, int dtype, unetdc_stream_t s);

/* ---- optimizer recipe: global-norm clipping, non-finite guard, decoupled weight decay, EMA -----
 * unetdc_step_ctl: the DEVICE-resident record unetdc_grad_norm writes and unetdc_adam_step_ex reads; the host never has to
 *   read it between the two.  The caller zeroes it once (steps, clipped, skipped and norm_sum accumulate over the calls;
 *   sumsq, norm, gscale_eff and skip are rewritten by every call, nothing of the previous step survives).
 * unetdc_grad_norm: sumsq = grad_scale^2 * sum_i flat_grad[i]^2 over i in [0, n), norm = sqrt(sumsq): the global L2 norm of
 *   grad_scale * flat_grad.  Two launches: at most 2048 fp64 partials (one per workgroup, 4096 elements per trip), then a
 *   one-workgroup finaliser.  Every product is formed as (double)g * (double)g, which is exact, and summed in fp64 in a fixed
 *   order: no atomics, no hand-off between workgroups, bitwise reproducible, and the relative error of sumsq is below
 *   (n + 2) 2^-53.  16-byte loads with a scalar tail: n need not be a multiple of 4.  Then
 *     skip = 1 when sumsq is not finite (an inf or NaN gradient anywhere), else 0;
 *     coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), 1 when max_norm <= 0 (no clipping);
 *     gscale_eff = (float)(grad_scale * coef), formed in double and rounded once (0 when skip is set);
 *     steps += 1; skipped += skip; on a finite step norm_sum += norm and clipped += (coef < 1).
 *   Nothing but the workspace (unetdc_grad_norm_workspace(n) bytes, 8-byte aligned; 0 for n <= 0) and the record is written.
 *   UNETDC_EINVAL before any HIP call: a null pointer, a flat_grad that is not 16-byte aligned, a ctl_dev or workspace that
 *   is not 8-byte aligned, n <= 0, a non-finite grad_scale, a NaN max_norm; UNETDC_EWORKSPACE for a workspace too small.
 * unetdc_adam_step_ex: unetdc_adam_step (same table, same work decomposition, the other instantiation of the same kernel) with
 *     ctl_dev (nullable): every workgroup reads the record once; with skip set it returns before touching anything (p, m, v,
 *       both images and the EMA stay bit for bit), else gscale_eff replaces (float)grad_scale;
 *     weight_decay: p <- p * (float)(1 - lr * weight_decay) before the Adam update, one extra rounding (torch.optim.AdamW),
 *       for the descriptors with bit 0 of `flags` set only;
 *     ema_base (nullable), m_base, ema_decay: the moving average of tensor i lives at ema_base + (table[i].m - m_base), i.e.
 *       in the flat layout of the moments; e <- e + (float)(1 - ema_decay) * (p_new - e), two roundings.
 *   The images are written from the new p.  With ctl_dev == NULL (or a record with gscale_eff == (float)grad_scale),
 *   weight_decay == 0 and ema_base == NULL the results equal unetdc_adam_step's bit for bit.  Refuses what unetdc_adam_step
 *   refuses, a weight_decay outside [0, 1 / lr), an ema_decay outside [0, 1], an ema_base without m_base. */
typedef struct unetdc_step_ctl {
  double sumsq, norm;
  float gscale_eff;
  int32_t skip;
  int64_t steps, clipped, skipped;
  double norm_sum;
} unetdc_step_ctl;
int64_t unetdc_grad_norm_workspace(int64_t n);
int unetdc_grad_norm(const float* flat_grad, int64_t n, double grad_scale, double max_norm, unetdc_step_ctl* ctl_dev,
                     void* workspace, int64_t workspace_bytes, unetdc_stream_t s);
int unetdc_adam_step_ex(const unetdc_adam_desc* table_dev, int n, int64_t total_blocks, const float* flat_grad, double lr,
                        double beta1, double beta2, double eps, int64_t step, double grad_scale, int dtype,
                        const unetdc_step_ctl* ctl_dev, double weight_decay, float* ema_base, const float* m_base,
                        double ema_decay, unetdc_stream_t s);

/* ---- dilated 3x3 convolution, padding = dilation: nn.Conv2d at models/model_2.py:41-44,48-51 ---
 * y = conv(x) + bias                                  (scale == NULL; training: raw pre-BN output)
 * y = relu(conv(x)*scale + shift)                     (scale != NULL; eval: BN folded, bias inside shift)
 * stats_part (nullable, training): per-block partial [rows][2][Cout] sums / sums of squares of y
 * as stored, rows = unetdc_conv3x3_stats_rows(); the buffer must hold rows+64 rows.
 * Cin must be a multiple of 64 (bf16) / 32 (fp32) and Cout of 64: every layer but enc1.0. */
int unetdc_conv3x3_stats_rows(int64_t npixels, int cout);
/* stats_rows (out, nullable; written when stats_part is given): rows of the statistics buffer that carry data
 * (<= unetdc_conv3x3_stats_rows(): the persistent kernels write one row per workgroup and zeros into the rest, so
 * summing all rows stays valid; passing this count to unetdc_bn_finalize saves it reading the zero rows). */
int unetdc_conv3x3_fwd(const void* x, int ldx, const void* w_fwd, const float* bias, const float* scale,
                       const float* shift, void* y, int ldy, float* stats_part, int* stats_rows, int n, int h, int w,
                       int cin, int cout, int dilation, int dtype, unetdc_stream_t s);
/* "bnin" forms (round 3): the convolution / weight gradient are fed from the RAW conv output of the stage in front of them and
 * apply that stage's BatchNorm + ReLU -- relu(in_scale * x + in_shift), models/model_2.py:45-46, rounded through the storage
 * type like a stored activation -- once per staged tile in LDS: the stand-alone unetdc_bn_relu_apply pass of that stage
 * disappears; outputs are bit-identical to the two-pass form.  bf16 only, shapes the persistent lattice kernel takes.
 * unetdc_conv3x3_bnin_supported() returns 0 (no), 1 (64-channel output blocks: forward + unetdc_conv3x3_wgrad_bnin, the activation
 * tensor is never stored) or 2 (round 5, 128-channel output blocks: the forward ALSO stores the normalised activation into
 * act_out [n*h*w][ldact] on request -- the bytes the stand-alone pass would have written, without its read of x and without its
 * launch -- so that any weight-gradient kernel can follow; act_out must be NULL where the answer is 1).
 * fwd: statistics mode only (training); in_scale / in_shift [cin] are the producing stage's batch scale / shift. */
int unetdc_conv3x3_bnin_supported(int n, int h, int w, int cin, int cout, int dilation, int dtype);
int unetdc_conv3x3_fwd_bnin(const void* x_raw, int ldx, const float* in_scale, const float* in_shift, const void* w_fwd,
                            const float* bias, void* y, int ldy, float* stats_part, int* stats_rows, void* act_out, int ldact,
                            int n, int h, int w, int cin, int cout, int dilation, int dtype, unetdc_stream_t s);
int unetdc_conv3x3_wgrad_bnin(const void* x_raw, int ldx, const float* in_scale, const float* in_shift, const void* dy,
                              int lddy, float* dw, void* workspace, int64_t workspace_bytes, int n, int h, int w, int cin,
                              int cout, int dilation, int dtype, unetdc_stream_t s);
/* dx = conv_transpose(dy): autograd of the above w.r.t. its input (dx has cin channels). */
int unetdc_conv3x3_dgrad(const void* dy, int lddy, const void* w_dgrad, void* dx, int lddx, int n, int h, int w,
                         int cin, int cout, int dilation, int dtype, unetdc_stream_t s);
/* dw [Cout][Cin][3][3] fp32 = sum over pixels; workspace >= unetdc_conv3x3_wgrad_workspace() bytes. */
int64_t unetdc_conv3x3_wgrad_workspace(int n, int h, int w, int cin, int cout, int dtype);
int unetdc_conv3x3_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, void* workspace,
                         int64_t workspace_bytes, int n, int h, int w, int cin, int cout, int dilation, int dtype,
                         unetdc_stream_t s);

/* ---- first encoder convolution (small Cin, reads the NCHW fp32 image): model_2.py:10 (enc1.0) ---
 * w is the fp32 PyTorch-layout parameter itself.  Same scale/shift/stats semantics as above. */
int unetdc_conv3x3_first_stats_rows(int64_t npixels, int cin, int cout);
int unetdc_conv3x3_first_fwd(const float* x_nchw, const float* w, const float* bias, const float* scale,
                             const float* shift, void* y, int ldy, float* stats_part, int n, int h, int wd, int cin,
                             int cout, int dilation, int dtype, unetdc_stream_t s);
int64_t unetdc_conv3x3_first_wgrad_workspace(int n, int h, int w, int cin, int cout);
int unetdc_conv3x3_first_wgrad(const float* x_nchw, const void* dy, int lddy, float* dw, void* workspace,
                               int64_t workspace_bytes, int n, int h, int w, int cin, int cout, int dilation,
                               int dtype, unetdc_stream_t s);
/* The first layer's weight gradient with the BatchNorm + ReLU backward of its stage applied ON LOAD (models/model_2.py:41-46
 * under autograd): dz = gradient of the stage's activated output, y = its saved conv output, coeffs [3][cout] from
 * unetdc_bn_relu_bwd_coeffs (which also finalises dgamma / dbeta / dbias from the partial sums a fused dgrad epilogue left:
 * unetdc_conv3x3_dgrad_bnstats).  dy = k1 * [a > 0] * dz - k2 - k3 * xhat is formed per loaded chunk, rounded through the
 * storage type -- bit-identical to unetdc_bn_relu_bwd + unetdc_conv3x3_first_wgrad, without the pass that writes dy and the
 * one that reads it.  Only when nothing else needs dy (no dL/dx) and for the shapes _supported answers 1 (one input channel,
 * dilation 1, w % 8 == 0). */
int unetdc_conv3x3_first_wgrad_bn_supported(int n, int h, int w, int cin, int cout, int dilation, int dtype);
int unetdc_bn_relu_bwd_coeffs(const float* pre_parts, int pre_nparts, const float* gamma, const float* rstd, float* dgamma,
                              float* dbeta, float* dbias, float* coeffs, int n, int h, int w, int c, unetdc_stream_t s);
int unetdc_conv3x3_first_wgrad_bn(const float* x_nchw, const void* dz, int lddz, const void* y, int ldy, const float* scale,
                                  const float* shift, const float* mean, const float* rstd, const float* coeffs, float* dw,
                                  void* workspace, int64_t workspace_bytes, int n, int h, int w, int cin, int cout,
                                  int dilation, int dtype, unetdc_stream_t s);
/* Gradient with respect to the INPUT image, dL/dx of the module's forward (autograd of the first nn.Conv2d, models/model_2.py:
 * 10,41-44,58; the reference's loops never request it, a saliency-style caller does): dx NCHW fp32 [n][cin][h][w] from the
 * gradient dy [n*h*w][lddy] of the first convolution's output and its fp32 weights in PyTorch layout [cout][cin][3][3]. */
int unetdc_conv3x3_first_dgrad(const void* dy, int lddy, const float* w, float* dx_nchw, int n, int h, int wd, int cin,
                               int cout, int dilation, int dtype, unetdc_stream_t s);

/* ---- ConvTranspose2d(k=2, s=2): models/model_2.py:20,23,26,29 and :67,70,73,76 -----------------
 * fwd: x [n,h,w,cin] -> up [n,2h,2w,cout] (+bias) written with pixel stride ldup (concat slice). */
int unetdc_convT2x2_fwd(const void* x, int ldx, const void* w_fwd, const float* bias, void* up, int ldup, int n,
                        int h, int w, int cin, int cout, int dtype, unetdc_stream_t s);
int unetdc_convT2x2_dgrad(const void* dup, int lddup, const void* w_dgrad, void* dx, int lddx, int n, int h, int w,
                          int cin, int cout, int dtype, unetdc_stream_t s);
int64_t unetdc_convT2x2_wgrad_workspace(int n, int h, int w, int cin, int cout, int dtype);
/* dw [Cin][Cout][2][2] fp32 (the bias gradient is unetdc_channel_sum of dup). */
int unetdc_convT2x2_wgrad(const void* x, int ldx, const void* dup, int lddup, float* dw, void* workspace,
                          int64_t workspace_bytes, int n, int h, int w, int cin, int cout, int dtype,
                          unetdc_stream_t s);

/* ---- BatchNorm2d + ReLU (+ max_pool2d): models/model_2.py:45-46,52-53 and :59-61,64 -------------
 * bn_finalize: batch statistics from the conv's partials -> scale = gamma*rstd,
 *   shift = beta - mean*scale, saved mean/rstd; running stats updated with momentum (unbiased var)
 *   when running_mean != NULL. `count` = n*h*w. */
int unetdc_bn_finalize(const float* stats_part, int rows, int64_t count, const float* gamma, const float* beta,
                       float eps, float momentum, float* running_mean, float* running_var, float* scale,
                       float* shift, float* mean, float* rstd, int c, unetdc_stream_t s);
/* eval: scale = gamma/sqrt(running_var+eps), shift = beta + (conv_bias - running_mean)*scale */
int unetdc_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, const float* conv_bias, float eps, float* scale, float* shift,
                          int c, unetdc_stream_t s);
/* a = relu(scale*y + shift) (a = y when scale == NULL); pooled (nullable) = max_pool2d(a, 2).
 * `a` may be NULL when only the pooled tensor is wanted and scale == NULL. */
int unetdc_bn_relu_apply(const void* y, int ldy, const float* scale, const float* shift, void* a, int lda,
                         void* pooled, int ldp, int n, int h, int w, int c, int dtype, unetdc_stream_t s);
/* backward of conv-output y -> BN(train) -> ReLU (-> skip and/or 2x2 max-pool consumers):
 *   incoming gradient = dskip (nullable, full resolution) + scatter(dpool) (nullable, half
 *   resolution, routed to the window arg-max recomputed from y); outputs dy (gradient of the conv
 *   output), dgamma, dbeta and the conv-bias gradient dbias (nullable).
 *   pre_parts (nullable, non-pooled form only): [pre_nparts][3][c] partial sums already produced by
 *   the *_dgrad_bnstats call that wrote dskip -- the reduction pass over (dskip, y) is then skipped.
 *   The buffer must have 64 spare rows after pre_nparts. */
int64_t unetdc_bn_relu_bwd_workspace(int n, int h, int w, int c, int pooled, int dtype);
int unetdc_bn_relu_bwd(const void* dskip, int ldskip, const void* dpool, int ldpool, const void* y, int ldy,
                       const float* scale, const float* shift, const float* mean, const float* rstd,
                       const float* gamma, void* dy, int lddy, float* dgamma, float* dbeta, float* dbias,
                       void* workspace, int64_t workspace_bytes, const float* pre_parts, int pre_nparts, int n, int h,
                       int w, int c, int dtype, unetdc_stream_t s);
/* unetdc_bn_relu_bwd for the stage in front of a ONE-channel head (dec1's second stage, models/model_2.py:76-80): the
 * gradient of the head's input is dz * w[c] with dz = dprobs * p * (1 - p) per pixel, so it is recomputed from the fp32
 * [N, 1, H, W] tensors instead of being written by unetdc_head_bwd_bnstats (call that with da = NULL) and read back -- two
 * activation-sized transfers less per step; rounded through the storage type, i.e. bit-identical to the stored form.
 * pre_parts / pre_nparts: the sums unetdc_head_bwd_bnstats produced (required). */
int unetdc_bn_relu_bwd_head(const float* dprobs, const float* probs, const float* head_w, const void* y, int ldy,
                            const float* scale, const float* shift, const float* mean, const float* rstd,
                            const float* gamma, void* dy, int lddy, float* dgamma, float* dbeta, float* dbias,
                            void* workspace, int64_t workspace_bytes, const float* pre_parts, int pre_nparts, int n, int h,
                            int w, int c, int dtype, unetdc_stream_t s);
/* BatchNorm with FROZEN statistics under autograd -- model.eval() with gradients enabled, i.e. fine-tuning with fixed
 * running statistics, which the reference module supports through plain autograd (nn.BatchNorm2d in eval mode,
 * models/model_2.py:45,52): unetdc_bn_frozen_affine fills scale / shift / mean / rstd from the running buffers (the conv bias
 * is added by the conv epilogue as in training), the forward then uses the training-path kernels; unetdc_bn_relu_bwd_frozen is
 * unetdc_bn_relu_bwd for that case: dy = gamma * rstd * dyhat (no batch terms), dgamma = sum dyhat * xhat, dbeta = sum dyhat,
 * dbias = sum dy. */
int unetdc_bn_frozen_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                            float eps, float* scale, float* shift, float* mean, float* rstd, int c, unetdc_stream_t s);
int unetdc_bn_relu_bwd_frozen(const void* dskip, int ldskip, const void* dpool, int ldpool, const void* y, int ldy,
                              const float* scale, const float* shift, const float* mean, const float* rstd,
                              const float* gamma, void* dy, int lddy, float* dgamma, float* dbeta, float* dbias,
                              void* workspace, int64_t workspace_bytes, const float* pre_parts, int pre_nparts, int n, int h,
                              int w, int c, int dtype, unetdc_stream_t s);
/* dgrad fused with the BatchNorm-backward REDUCTION of the stage that consumes dx: besides dx the
 * kernel epilogue accumulates, per channel of dx, S1 = sum dx*[n>0] and S2 = sum dx*[n>0]*xhat with
 * n = scale*y_prev + shift, xhat = (y_prev - mean)*rstd (y_prev = that stage's saved conv output, same
 * pixel grid as dx).  parts: [*nparts][3][cin] fp32 (third row zero), parts_floats >= (rows+64)*3*cin
 * with rows = unetdc_conv3x3_stats_rows(n*h*w, cin); *nparts receives the rows written.  The y_prev
 * read overlaps with matrix-core work here instead of costing a separate HBM pass. */
int unetdc_conv3x3_dgrad_bnstats(const void* dy, int lddy, const void* w_dgrad, void* dx, int lddx,
                                 const void* y_prev, int ldy_prev, const float* scale, const float* shift,
                                 const float* mean, const float* rstd, float* parts, int64_t parts_floats,
                                 int* nparts, int n, int h, int w, int cin, int cout, int dilation, int dtype,
                                 unetdc_stream_t s);
int unetdc_convT2x2_dgrad_bnstats(const void* dup, int lddup, const void* w_dgrad, void* dx, int lddx,
                                  const void* y_prev, int ldy_prev, const float* scale, const float* shift,
                                  const float* mean, const float* rstd, float* parts, int64_t parts_floats,
                                  int* nparts, int n, int h, int w, int cin, int cout, int dtype, unetdc_stream_t s);

/* ---- head: Conv2d(C, OC, 1) + sigmoid, models/model_2.py:32,79-80 ------------------------------
 * w [OC][C] fp32, probs/dprobs NCHW fp32 [n][OC][h][w]. */
int unetdc_head_fwd(const void* a, int lda, const float* w, const float* b, float* probs, int n, int h, int wd,
                    int c, int oc, int dtype, unetdc_stream_t s);
/* The same head fed from the RAW conv output y of the stage in front of it (dec1's second stage, models/model_2.py:76-79):
 * that stage's BatchNorm + ReLU, a = relu(scale * y + shift) (models/model_2.py:52-53), is applied while loading, rounded
 * through the storage type like a stored activation would be -- the activation tensor itself is never written or read
 * (train-mode forward; the eval-mode convolution folds BatchNorm into its own epilogue and feeds unetdc_head_fwd). */
int unetdc_head_fwd_bn(const void* y, int ldy, const float* scale, const float* shift, const float* w, const float* b,
                       float* probs, int n, int h, int wd, int c, int oc, int dtype, unetdc_stream_t s);
int64_t unetdc_head_bwd_workspace(int n, int h, int w, int c, int oc, int dtype);
int unetdc_head_bwd(const float* dprobs, const float* probs, const void* a, int lda, const float* w, void* da,
                    int ldda, float* dw, float* db, void* workspace, int64_t workspace_bytes, int n, int h, int wd,
                    int c, int oc, int dtype, unetdc_stream_t s);
/* head_bwd that also produces the BatchNorm-backward partial sums of the stage whose activated output `a` is (the
 * block feeding out_conv, models/model_2.py:76-79), in the layout unetdc_bn_relu_bwd takes as pre_parts: the
 * gradient da is then read once by that stage's backward instead of twice.  y_prev/scale/shift/mean/rstd: that
 * stage's saved conv output and batch statistics; parts needs (rows + 64) * 3 * c floats, *nparts receives rows.
 * a == NULL: the activation is recomputed from y_prev / scale / shift (the counterpart of unetdc_head_fwd_bn). */
int unetdc_head_bwd_bnstats(const float* dprobs, const float* probs, const void* a, int lda, const float* w, void* da,
                            int ldda, float* dw, float* db, void* workspace, int64_t workspace_bytes, const void* y_prev,
                            int ldy_prev, const float* scale, const float* shift, const float* mean, const float* rstd,
                            float* parts, int64_t parts_floats, int* nparts, int n, int h, int wd, int c, int oc, int dtype,
                            unetdc_stream_t s);

/* ---- fused Focal + Dice loss on probabilities: utils/metrics_DC.py:65-73 (FocalLoss :43-63, dice_loss :11-17) ---
 * probs/target: fp32 [nimg][hw] (nimg = N*C maps, hw pixels each).  fwd writes the scalar loss and the
 * per-map coefficients {2/(U+s), (2I+s)/(U+s)^2} that bwd needs; bwd writes
 * dprobs = grad_out[0] * d loss / d probs.  alpha/gamma: focal parameters; ratio: focal weight;
 * smooth: the Dice smoothing constant (1e-7 in the reference). */
int64_t unetdc_focal_dice_loss_workspace(int nimg, int64_t hw);
int unetdc_focal_dice_loss_fwd(const float* probs, const float* target, float* loss_out, float* coef, void* workspace,
                               int64_t workspace_bytes, int nimg, int64_t hw, float alpha, float gamma, float ratio,
                               float smooth, unetdc_stream_t s);
int unetdc_focal_dice_loss_bwd(const float* probs, const float* target, const float* coef, const float* grad_out,
                               float* dprobs, int nimg, int64_t hw, float alpha, float gamma, float ratio,
                               unetdc_stream_t s);

/* ---- border-weighted loss (border.hip, loss.hip; the definition is DESIGN.md section 19, utils/border_weights.py) -----------
 * unetdc_border_weights: target ([n][h][w] fp32, foreground where > 0.5; the images are independent) ->
 *   out_weight ([n][h][w] fp32).  With the 4-connected components of an image (the connectivity of unetdc_ccl_stats), for a
 *   background pixel x:  D1 = the smallest squared Euclidean distance to a foreground pixel with |dy| <= radius and
 *   |dx| <= radius, D2 = the smallest to such a pixel of another component than that one (D2 = D1 when two components tie),
 *   UNETDC_EDT_INF where nothing qualifies; foreground pixels have D1 = D2 = 0.
 *     out_weight = 1 + w0 * exp(-(sqrt(D1) + sqrt(D2))^2 / (2 sigma^2))   on background pixels with D2 <= radius^2
 *                  (there D1 and D2 are the distances of the untruncated transform), exactly 1.0f everywhere else.
 *   out_d1 / out_d2 (nullable, [n][h][w] int32): the planes D1, D2.
 *   n 1..65535, sides 1..16384, h * w < 2^30, radius 1..64, sigma > 0, w0 >= 0 (both finite); anything else, a null target /
 *   out_weight / workspace or a workspace that is not 4-byte aligned returns UNETDC_EINVAL before the first launch, a workspace
 *   below unetdc_border_weights_workspace(n, h, w, radius) bytes (14 per pixel + 64; 0 for a geometry the call refuses)
 *   UNETDC_EWORKSPACE.  Nothing but the outputs and the workspace is written, whatever the workspace held; no allocation, no
 *   host wait; launches on the given stream only.  Integer work and a union-find up to the final expression: the planes depend
 *   on no order, two runs are bitwise equal in all three outputs.
 * unetdc_focal_dice_loss_w_fwd / _w_bwd: unetdc_focal_dice_loss_fwd / _bwd with weight ([nimg][hw] fp32, not differentiated)
 *   on the pixel-wise term only:  loss = ratio * sum_j(weight_j * focal_j) / (nimg * hw) + (1 - ratio) * (1 - mean_i dice_i),
 *   dprobs_j = g * (ratio / (nimg * hw) * weight_j * dfocal_j - (1 - ratio) / nimg * (t_j c1 - c2)).  The same kernel bodies:
 *   a weight of 1.0f everywhere gives the bits of the unweighted calls.  Workspace: unetdc_focal_dice_loss_workspace. */
int64_t unetdc_border_weights_workspace(int n, int h, int w, int radius);
int unetdc_border_weights(const float* target, int n, int h, int w, float w0, float sigma, int radius, float* out_weight,
                          int32_t* out_d1, int32_t* out_d2, void* workspace, int64_t workspace_bytes, unetdc_stream_t s);
int unetdc_focal_dice_loss_w_fwd(const float* probs, const float* target, const float* weight, float* loss_out, float* coef,
                                 void* workspace, int64_t workspace_bytes, int nimg, int64_t hw, float alpha, float gamma,
                                 float ratio, float smooth, unetdc_stream_t s);
int unetdc_focal_dice_loss_w_bwd(const float* probs, const float* target, const float* weight, const float* coef,
                                 const float* grad_out, float* dprobs, int nimg, int64_t hw, float alpha, float gamma,
                                 float ratio, unetdc_stream_t s);

/* conv3x3_dgrad that also returns colsum[i] = sum over pixels of the STORED dx[:, c0 + i], i < c (fp32).
 * The decoder's first conv writes the gradient of torch.cat([up, enc]) (models/model_2.py:68,71,74,77); the
 * column sums of its first half are the ConvTranspose2d bias gradient (:20,23,26,29), so that gradient costs
 * no extra pass over the tensor. */
int64_t unetdc_conv3x3_dgrad_colsum_workspace(int n, int h, int w, int cin);
int unetdc_conv3x3_dgrad_colsum(const void* dy, int lddy, const void* w_dgrad, void* dx, int lddx, float* colsum, int c0,
                                int c, void* workspace, int64_t workspace_bytes, int n, int h, int w, int cin, int cout,
                                int dilation, int dtype, unetdc_stream_t s);

/* ---- per-channel column sum of an NHWC tensor (ConvTranspose2d bias gradient) ------------------ */
int64_t unetdc_channel_sum_workspace(int64_t npixels, int c);
int unetdc_channel_sum(const void* x, int ldx, float* out, void* workspace, int64_t workspace_bytes,
                       int64_t npixels, int c, int dtype, unetdc_stream_t s);

/* ---- droplet quantification: /root/reference/quantify_droplets_batch.py:56-57,81-95 ----------
 * unetdc_mask_from_probs: mask[y][x] = probs[sy][sx] > thresh (strict, fp32) with the nearest-neighbour index rule of
 *   cv2.resize(..., INTER_NEAREST): s = min(floor(d * src/dst), src-1); probs [ph][pw] fp32 (one image, one channel),
 *   mask [oh][ow] uint8 {0,1}.
 * unetdc_ccl_stats: 4-connected components of a {0,1} mask, objects smaller than min_area dropped, the rest numbered in
 *   raster order of their first pixel (= skimage.measure.label twice + regionprops order).  Outputs, per kept object in
 *   that order: out_area (pixels), out_sumy / out_sumx (sums of row / column indices: centroid = sum / area),
 *   out_root (linear index of the first pixel; may be NULL); *out_count = number of kept objects (may exceed max_out:
 *   only the first max_out are written).  All outputs are DEVICE pointers.  Exact integer arithmetic, order-independent. */
int unetdc_mask_from_probs(const float* probs, int ph, int pw, float thresh, uint8_t* mask, int oh, int ow,
                           unetdc_stream_t s);
/* The mask the reference's call actually produces: `cv2.resize(mask512, (ow, oh), cv2.INTER_NEAREST)`
 * (/root/reference/quantify_droplets_batch.py:57) passes the flag in the positional slot of `dst`, so OpenCV's default
 * 8-bit INTER_LINEAR runs on the {0,1} mask.  Tables as for unetdc_resize_linear_u8_to_chw_f32. */
int unetdc_mask_from_probs_linear(const float* probs, int ph, int pw, float thresh, uint8_t* mask, int oh, int ow,
                                  const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                                  unetdc_stream_t s);
int64_t unetdc_ccl_workspace(int h, int w);
int unetdc_ccl_stats(const uint8_t* mask, int h, int w, int min_area, void* workspace, int64_t workspace_bytes,
                     int32_t* out_count, int32_t* out_area, int64_t* out_sumy, int64_t* out_sumx, int32_t* out_root,
                     int max_out, unetdc_stream_t s);

/* ---- input preprocessing: /root/reference/utils/data_loader.py:11-24, quantify_droplets_batch.py:40-46
 * unetdc_rolling_ball_u8: per channel of an interleaved HWC uint8 image: background = opening with the ksize x ksize
 *   ellipse of cv2.getStructuringElement (dilate(erode(.)), pixels outside the image ignored), dst = normalize_minmax(
 *   saturate(src - background)) to 0..255 (scale/shift in double, applied in float, round half to even).  ksize <= 128,
 *   channels <= 4.  dst may not alias src.  src, dst and the workspace must be 16-byte aligned: anything else returns
 *   UNETDC_EINVAL before the first launch.
 * unetdc_resize_linear_u8_to_chw_f32: OpenCV's 8-bit INTER_LINEAR resize to (dh, dw), / 255, HWC -> CHW float32 (the
 *   network input layout).  xofs[dw] / yofs[dh]: source index of the first tap (x already clamped to [0, w-1]),
 *   xcoef[dw][2] / ycoef[dh][2]: the 11-bit coefficients (utils/data_loader.py:linear_tables builds them). */
int64_t unetdc_rolling_ball_workspace(int h, int w, int channels);
int unetdc_rolling_ball_u8(const uint8_t* src_hwc, uint8_t* dst_hwc, int h, int w, int channels, int ksize, void* workspace,
                           int64_t workspace_bytes, unetdc_stream_t s);
int unetdc_resize_linear_u8_to_chw_f32(const uint8_t* src_hwc, int h, int w, int channels, float* dst_chw, int dh, int dw,
                                       const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                                       unetdc_stream_t s);

/* ---- training augmentation on a device-resident cache (utils/data_loader.py:TrainAugment restated; augment.hip) ------
 * unetdc_elastic_fields: for each of n field slots, the displacement pair of TrainAugment's elastic step,
 *   fields[i][0] = dx, fields[i][1] = dy, each [h][w] float32 = alpha * gaussian_filter(noise, sigma, mode="constant",
 *   truncate=4.0), where noise(seed, component, y, x) in [-1, 1) is a counter-based hash (no RNG state on the device):
 *     f(h) = murmur3 fmix32;  key = f(f(f(seed) ^ component * 0x9E3779B9) ^ y);  noise = (f(key ^ x) >> 8) * 2^-23 - 1.
 *   seeds: HOST array of n seeds (passed to the kernels by value).  h, w <= 1024; int(4 sigma + 0.5) <= 1024.
 * unetdc_augment_gather: out_img[i] ([c][h][w] float32) and out_mask[i] ([1][h][w] float32 in {0, 1}) for n samples, each
 *   made from cache_img[params[i].src] ([ncache][c][h][w] float32) and cache_mask[params[i].src] ([ncache][h][w] uint8) by
 *   hflip, vflip, np.rot90(k, axes (0, 1)), brightness / contrast clip(alpha * x + beta_max, 0, 1) (two float32 roundings,
 *   no FMA) and, when params[i].field >= 0, the elastic warp with the fields of that slot (image: bilinear, mask: nearest,
 *   both with scipy.ndimage's mode "reflect").  params: HOST array of n records.  An odd k needs h == w. */
#define UNETDC_AUG_HFLIP 1
#define UNETDC_AUG_VFLIP 2
#define UNETDC_AUG_BC 4
typedef struct unetdc_augment_params {
  int32_t src;          /* index into the cache */
  int32_t flags;        /* UNETDC_AUG_* bits */
  int32_t k;            /* 90-degree rotations, 0..3 */
  int32_t field;        /* field slot, -1 = no elastic */
  float alpha;          /* contrast factor, float32(alpha) */
  float beta_max;       /* float32(beta * max of the source image), the product formed in double */
  int32_t reserved[2];
} unetdc_augment_params;
int64_t unetdc_elastic_fields_workspace(int n, int h, int w, double sigma);
int unetdc_elastic_fields(const uint32_t* seeds, int n, int h, int w, double sigma, float alpha, float* fields,
                          void* workspace, int64_t workspace_bytes, unetdc_stream_t s);
int unetdc_augment_gather(const float* cache_img, const uint8_t* cache_mask, int ncache, int channels, int h, int w,
                          const unetdc_augment_params* params, int n, const float* fields, int nfields, float* out_img,
                          float* out_mask, unetdc_stream_t s);

/* ---- training at native resolution: random crops of images cached at their own size (crop.hip) ----
 * unetdc_crop_gather: out_img[i] ([channels][S][S] float32) and out_mask[i] ([1][S][S] float32) for n samples.  Sample i reads
 *   the HWC uint8 image of params[i].h x params[i].w pixels at images_u8 + params[i].img_off and the uint8 mask of the same
 *   size at masks_u8 + params[i].mask_off (two flat DEVICE buffers of images_bytes / masks_bytes bytes that hold every cached
 *   image back to back).  The window is win[c][y][x] = float(img[fold(y0 + y, h)][fold(x0 + x, w)][c]) / 255.0f (one IEEE
 *   division; fold: the reflect-101 rule of unetdc_tile_gather_u8_to_chw_f32, which only an image smaller than S along an
 *   axis ever needs) and the mask window the mask bytes at the same pixels; the output is what unetdc_augment_gather makes of
 *   that S x S window: hflip, vflip, np.rot90(k), clip(alpha * x + beta_max, 0, 1) (two float32 roundings, no FMA) and, when
 *   params[i].field >= 0, the elastic warp with fields[field] ([nfields][2][S][S] float32 of unetdc_elastic_fields at S x S),
 *   reflected at the WINDOW's border.  utils/crops.py:crop_gather_numpy is the same rule on the host, bit-equal without
 *   elastic.  params: HOST array of n records, passed to the kernel by value: nothing but the two outputs is written, no
 *   workspace, no allocation, no host wait, no atomics; launches on the given stream only.
 *   UNETDC_EINVAL before any launch: a null pointer (fields may be null when no record has a field), S not a multiple of 16
 *   in 16..1024, channels outside 1..4, a side outside 1..16384, y0 / x0 outside 0..max(side - S, 0), img_off + h * w *
 *   channels > images_bytes or mask_off + h * w > masks_bytes (or a negative offset), k outside 0..3, unknown flags, a field
 *   slot outside [-1, nfields).  Every coordinate is folded, so every read of an accepted record lies inside its image. */
typedef struct unetdc_crop_params {
  int64_t img_off;      /* byte offset of the image in images_u8 */
  int64_t mask_off;     /* byte offset of the mask in masks_u8 */
  int32_t h, w;         /* the image's own size */
  int32_t y0, x0;       /* window origin */
  int32_t flags;        /* UNETDC_AUG_* bits */
  int32_t k;            /* 90-degree rotations, 0..3 */
  int32_t field;        /* field slot, -1 = no elastic */
  float alpha;          /* contrast factor, float32(alpha) */
  float beta_max;       /* float32(beta * max of the whole cached image / 255), the product formed in double */
  int32_t reserved;     /* pads the record to 56 bytes */
} unetdc_crop_params;
int unetdc_crop_gather(const uint8_t* images_u8, int64_t images_bytes, const uint8_t* masks_u8, int64_t masks_bytes, int channels,
                       int S, const unetdc_crop_params* records, int n, const float* fields, int nfields, float* out_img,
                       float* out_mask, unetdc_stream_t s);

/* unetdc_crop_gather_scaled: unetdc_crop_gather with scale jitter.  Sample i cuts the t x t SOURCE window at (y0, x0) of its
 *   image (the window rule above with t in place of S) and resamples it to the S x S lattice in the same pass:
 *   - image: OpenCV's 8-bit INTER_LINEAR, as utils.data_loader.resize_linear_cv2_u8(window, S, S).  Per lattice coordinate d
 *     the taps of linear_tables(t, S): f = (d + 0.5) * (double(t) / double(S)) - 0.5 in double (two roundings, no FMA), first
 *     tap floor(f), coefficients rint((1.0f - float(frac)) * 2048) and rint(float(frac) * 2048).  Along x a first tap below 0
 *     or at / above t - 1 becomes one tap of weight 2048; along y both taps are clamped to 0..t-1 and keep their weights.
 *     Then r = p0 * a0 + p1 * a1 per source row and v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, all in
 *     int32, and the lattice value float(v) / 255.0f.  The resize acts in the window's own orientation, before flips / rot90.
 *   - mask: the source mask at min(floor(d * (double(t) / double(S))), t - 1) on both axes (INTER_NEAREST).
 *   The output is what unetdc_crop_gather makes of that lattice (flips, rot90, brightness / contrast, elastic with the four
 *   bilinear lattice taps and the nearest mask tap; a lattice tap is a scaled pixel: 4 source bytes per channel, 16 with a
 *   field).  utils/crops.py:crop_gather_scaled_numpy is the same rule on the host, bit-equal without elastic; with t == S the
 *   outputs are those of unetdc_crop_gather bit for bit.  Records by value, nothing but the two outputs is written, no
 *   workspace, no allocation, no host wait, no atomics; launches on the given stream only.
 *   UNETDC_EINVAL before any launch: everything unetdc_crop_gather refuses, with y0 / x0 taken against 0..max(side - t, 0),
 *   and t outside S / 2 .. 2 S.  Every tap is clamped to the window and then folded into the image, so every read of an
 *   accepted record lies inside its image. */
typedef struct unetdc_crop_scaled_params {
  int64_t img_off;      /* as unetdc_crop_params */
  int64_t mask_off;
  int32_t h, w;
  int32_t y0, x0;       /* origin of the t x t source window */
  int32_t flags;
  int32_t k;
  int32_t field;
  float alpha;
  float beta_max;
  int32_t t;            /* side of the source window, S / 2 .. 2 S (where unetdc_crop_params has `reserved`) */
} unetdc_crop_scaled_params;
int unetdc_crop_gather_scaled(const uint8_t* images_u8, int64_t images_bytes, const uint8_t* masks_u8, int64_t masks_bytes,
                              int channels, int S, const unetdc_crop_scaled_params* records, int n, const float* fields,
                              int nfields, float* out_img, float* out_mask, unetdc_stream_t s);


/* ---- radial and spatial droplet density maps (the reference's quantify_pipline.py:44-142 restated; density.hip) ---------
 * unetdc_density_maps: for one image of h x w pixels (both sides >= UNETDC_DENSITY_MIN_SIDE):
 *   roi      = cv2 RGB2GRAY -> GaussianBlur((15, 15), 0) in OpenCV's bit-exact 8-bit form (BORDER_REFLECT_101) -> Otsu ->
 *              MORPH_CLOSE then MORPH_OPEN with the 15 x 15 rectangle -> > 0;
 *   (cx, cy) = int(m10 / m00), int(m01 / m00) of roi, (w / 2, h / 2) when the ROI is empty;
 *   rings    = np.linspace(0, max ROI distance, nb_layers + 1); ring_count[i] = droplets whose centroid distance d has
 *              b_i < d <= b_{i+1} (droplets: the first min(*droplet_count, max_droplets) entries of unetdc_ccl_stats
 *              outputs, which must have been made with min_area = 1); the radial map paints ring_count[i] on ring i's ROI pixels;
 *   spatial  = gaussian_filter(mask, sigma) / (gaussian_filter(roi, sigma) + 1e-5) * 100 in float32 (scipy's mode
 *              "reflect", truncate 4: radius int(4 sigma + 0.5) <= UNETDC_DENSITY_MAX_RADIUS);
 *   index planes = min(int(normalize(map) * 256), 255), 0 for a constant map (the pixels of plt.imsave(cmap=...) are
 *              lut[index]).
 *   rgb_hwc: [h][w][3] uint8, mask: [h][w] uint8 {0, 1}; taps: HOST array of radius + 1 fp64 weights, centre first, as
 *   scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius)[radius:].  out_stats, out_radial_index and out_spatial_index
 *   ([h][w] uint8 each) are DEVICE pointers; out_blur, out_roi, out_ring (ring index + 1, 0 = none) [h][w] uint8 and
 *   out_radial, out_spatial [h][w] float32 are optional DEVICE outputs of the intermediate planes (NULL: kept in the workspace).
 *   1 <= nb_layers <= UNETDC_DENSITY_MAX_LAYERS.
 * unetdc_density_sqrt: out[i] = sqrt((double)x[i]) with the square root the density kernels use (DEVICE pointers). */
#define UNETDC_DENSITY_MIN_SIDE 2
#define UNETDC_DENSITY_MAX_LAYERS 255
#define UNETDC_DENSITY_MAX_RADIUS 128
typedef struct unetdc_density_stats {
  int64_t roi_area;            /* m00 */
  int64_t m10, m01;            /* sums of x and y over the ROI */
  int32_t cx, cy;              /* ROI centroid (truncated) */
  int32_t otsu_threshold;
  int32_t nb_layers;
  double max_ring_distance;    /* largest ROI pixel distance from (cx, cy); 0 for an empty ROI */
  int32_t ndroplets;           /* *droplet_count as read */
  uint32_t radial_min_bits, radial_max_bits, spatial_min_bits, spatial_max_bits;     /* float32 bit patterns */
  int32_t ring_count[UNETDC_DENSITY_MAX_LAYERS];
} unetdc_density_stats;
int64_t unetdc_density_workspace(int h, int w);
int unetdc_density_maps(const uint8_t* rgb_hwc, const uint8_t* mask, int h, int w, const int32_t* droplet_count,
                        const int32_t* droplet_area, const int64_t* droplet_sumy, const int64_t* droplet_sumx,
                        int max_droplets, int nb_layers, double sigma, const double* taps, void* workspace,
                        int64_t workspace_bytes, unetdc_density_stats* out_stats, uint8_t* out_radial_index,
                        uint8_t* out_spatial_index, uint8_t* out_blur, uint8_t* out_roi, uint8_t* out_ring,
                        float* out_radial, float* out_spatial, unetdc_stream_t s);
int unetdc_density_sqrt(const int64_t* x, double* out, int64_t n, unetdc_stream_t s);


/* ---- splitting touching droplets (split.hip; the definition is DESIGN.md, "Splitting touching droplets") -----------------
 * unetdc_edt_sq: out_d2[p] ([h][w] int32) = the exact squared Euclidean distance from pixel p of the uint8 mask [h][w]
 *   (nonzero = foreground) to the nearest zero pixel INSIDE the image, 0 on zero pixels (scipy.ndimage's
 *   distance_transform_edt convention: the outside of the image is not background).  A mask without any zero pixel has
 *   no finite distance: every pixel gets UNETDC_EDT_INF.  Sides 1..16384.  workspace: at least 4 * h * w + 64 bytes
 *   (unetdc_split_workspace(h, w) covers it).
 * unetdc_split_stats: the outputs of unetdc_ccl_stats (same meaning, same order rule, *out_count may exceed max_out) for
 *   the droplets that remain when every 4-connected component is cut along the saddles of its distance transform that
 *   lie deeper than split_depth_half_px / 2 pixels below the lower of the two peaks they separate:
 *     basins   every foreground pixel points to the largest key (D2, -index) among itself and its foreground
 *              4-neighbours; pixels whose chains end in the same pixel form a basin, peak = D2 there;
 *     merging  4-adjacent foreground pixels p, q of basins A != B are united iff, with S = min(D2[p], D2[q]),
 *              P = min(peak(A), peak(B)), H2 = split_depth_half_px:  t = 4P - 4S - H2^2 <= 0  or  t^2 <= 16 H2^2 S
 *              (that is sqrt(P) - sqrt(S) <= H2 / 2, in integers);
 *     droplets the classes of that union-find with at least max(min_area, 1) pixels, numbered in raster order of their
 *              first pixel.
 *   H2 >= 2 * ceil(sqrt(h^2 + w^2)) unites everything that touches: the outputs then equal unetdc_ccl_stats bit for bit.
 *   out_root (nullable): first-pixel index of each droplet; out_label (nullable): [h][w] int32, the 1-based number of
 *   the droplet of every pixel, 0 on background and on dropped droplets (numbers run past max_out).
 *   Sides 1..16384; split_depth_half_px >= 0; workspace: unetdc_split_workspace(h, w) bytes (0 for a non-positive side). */
#define UNETDC_EDT_INF 2147483647
int unetdc_edt_sq(const uint8_t* mask, int h, int w, int32_t* out_d2, void* workspace, int64_t workspace_bytes,
                  unetdc_stream_t s);
int64_t unetdc_split_workspace(int h, int w);
int unetdc_split_stats(const uint8_t* mask, int h, int w, int min_area, int split_depth_half_px, void* workspace,
                       int64_t workspace_bytes, int32_t* out_count, int32_t* out_area, int64_t* out_sumy, int64_t* out_sumx,
                       int32_t* out_root, int32_t* out_label, int max_out, unetdc_stream_t s);


/* ---- per-droplet shape and intensity integers (ccl.hip, shape.hip; the definition is DESIGN.md section 11) -----------------
 * unetdc_ccl_labels: the outputs of unetdc_ccl_stats (same meaning, same order rule, *out_count may exceed max_out, out_root
 *   nullable) plus out_label ([h][w] int32, required): the 1-based number of the droplet of every pixel, 0 on background
 *   and on components below min_area (numbers run past max_out), as unetdc_split_stats writes it.
 *   workspace: unetdc_ccl_labels_workspace(h, w) bytes (0 for a non-positive side).
 * unetdc_label_props: label ([h][w] int32: 0 = background, droplets 1..K; any label map, touching labels allowed) and
 *   optionally gray ([h][w] uint8, NULL = none) -> out[UNETDC_SHAPE_QUANTITIES][max_out] int64, row q of droplet k at
 *   out[q * max_out + k - 1]:
 *     0..2   Syy, Sxx, Sxy      sums of y^2, x^2, x * y over the droplet's pixels
 *     3..6   min_y, min_x, max_y, max_x   bounding box, inclusive
 *     7..9   P1, P2, P3         border pixels by perimeter class: a pixel of label k is a border pixel if one of its
 *                               4-neighbours lies outside the image or has another label; its code is 1 + 2 * (border
 *                               4-neighbours of label k) + 10 * (border diagonal neighbours of label k); P1 counts the codes
 *                               {5, 7, 15, 17, 25, 27}, P2 {21, 33}, P3 {13, 23}
 *                               (perimeter = P1 + sqrt(2) P2 + (1 + sqrt(2)) / 2 P3, applied by the caller)
 *     10..13 Sg, Sgg, min_g, max_g   sum, sum of squares, minimum, maximum of gray over the droplet's pixels
 *   Every row is initialised for all max_out droplets: sums and counts 0, minima INT64_MAX, maxima -1; that is what a
 *   number without pixels keeps, and what rows 10..13 keep when gray is NULL.  Labels below 1 or above max_out are
 *   skipped.  Sides 1..16384.  No workspace.  Integer atomics only: bitwise reproducible. */
#define UNETDC_SHAPE_QUANTITIES 14
int64_t unetdc_ccl_labels_workspace(int h, int w);
int unetdc_ccl_labels(const uint8_t* mask, int h, int w, int min_area, void* workspace, int64_t workspace_bytes,
                      int32_t* out_count, int32_t* out_area, int64_t* out_sumy, int64_t* out_sumx, int32_t* out_root,
                      int32_t* out_label, int max_out, unetdc_stream_t s);
int unetdc_label_props(const int32_t* label, const uint8_t* gray, int h, int w, int64_t* out, int max_out,
                       unetdc_stream_t s);


/* ---- per-droplet confidence and TTA disagreement (confidence.hip; the definition is DESIGN.md section 23) -------------------
 * unetdc_label_confidence: label ([h][w] int32: 0 = background, droplets 1..max_out; any label map, touching labels allowed),
 *   probs ([ph][pw] fp32) and optionally the envelope lo, hi ([ph][pw] fp32 each: the per-pixel minimum and maximum over the
 *   variants of unetdc_dihedral_mean_env_f32; both NULL or both given).  Pixel (y, x) reads the planes at
 *   (min(floor(y * ph / h), ph - 1), min(floor(x * pw / w), pw - 1)), the index rule of unetdc_mask_from_probs.  Per pixel:
 *     q = rint(clamp(p, 0, 1) * 65535), the product in fp32, ties to even, a NaN gives 0; H = entropy_table[q] (uint16 [65536],
 *     utils.droplet_confidence.entropy_table: rint(65535 * binary entropy in bits)); uncertain = |q - q(thresh)| <= q(band);
 *     spread = q(hi) - q(lo); unstable = !(lo > thresh) && hi > thresh.
 *   -> out[UNETDC_CONF_QUANTITIES][max_out] int64, row j of droplet k at out[j * max_out + k - 1]:
 *     0 n, 1 Sq, 2 Sqq (sums of 1, q, q^2), 3 min_q, 4 max_q, 5 n_band (uncertain pixels), 6 Sh (sum of H),
 *     7 Sspread, 8 max_spread, 9 n_unstable
 *   Every row is initialised for all max_out droplets: sums and counts 0, minima INT64_MAX, maxima -1; that is what a number
 *   without pixels keeps, and what rows 7..9 keep without an envelope.  Labels below 1 or above max_out are skipped there.
 *   -> out_image[UNETDC_CONF_IMAGE_QUANTITIES] int64 (required): 0 n_px (= h * w), 1 n_fg (label > 0, whatever max_out),
 *     2 Sh_all, 3 Sh_fg (H over all / foreground pixels), 4 n_band_all, 5 n_band_fg, 6 n_unstable_all, 7 Sspread_all (6 and 7
 *     stay 0 without an envelope).
 *   -> out_entropy_u8, out_spread_u8 ([h][w] uint8, each nullable): H >> 8 and spread >> 8; the spread map needs an envelope.
 *   out may be NULL when max_out == 0.  Sides 1..16384 with h * w < 2^30; ph, pw >= 1; 0 <= band <= 0.5.  No workspace; nothing
 *   but the outputs is written, and they may hold anything on entry.  Integer atomics only: bitwise reproducible.
 *   UNETDC_EINVAL before any launch: a null pointer, one of lo / hi alone, a spread map without an envelope, a side or band
 *   outside the limits. */
#define UNETDC_CONF_QUANTITIES 10
#define UNETDC_CONF_IMAGE_QUANTITIES 8
int unetdc_label_confidence(const int32_t* label, int max_out, int h, int w, const float* probs, const float* lo,
                            const float* hi, int ph, int pw, float thresh, float band, const uint16_t* entropy_table,
                            int64_t* out, int64_t* out_image, uint8_t* out_entropy_u8, uint8_t* out_spread_u8,
                            unetdc_stream_t s);


/* ---- convex hull, solidity and Feret integers per droplet (hull.hip; the definition is DESIGN.md section 24) -----------------
 * unetdc_label_hull: label ([h][w] int32: 0 = background, droplets 1..max_out; any label map: labels may touch and need not be
 *   connected; values below 1 or above max_out are skipped).  The point set of label k is the union of the closed unit squares
 *   [x, x + 1] x [y, y + 1] of its pixels (y, x); its convex hull has lattice vertices in 0..w x 0..h and is taken without
 *   collinear points, so a label with a pixel has at least 4 vertices and area >= 1.
 *   -> out[UNETDC_HULL_QUANTITIES][max_out] int64, row j of droplet k at out[j * max_out + k - 1]:
 *     0 H2   twice the hull's area (shoelace sum)
 *     1 F2   the largest squared distance between two hull vertices (Feret maximum squared)
 *     2 Wc   of the minimising edge e = (p -> q): max over vertices v of |e x (v - p)|
 *     3 Wl   that edge's squared length |e|^2
 *     4 nv   number of hull vertices
 *   The minimising edge is the one with the smallest Wc^2 / Wl (the squared caliper width across it), compared exactly by
 *   cross-multiplication in 128 bits; among equal ratios the one with the smallest Wl, which makes (Wc, Wl) unique.  A number
 *   without pixels keeps 0 in all five rows.
 *   *out_rows = the number of row-extent slots needed: the sum over the labels with pixels of max_y - min_y + 1.  If that
 *   exceeds max_rows, *out_rows = max_rows + 1 and out is unspecified (nothing outside it is written): repeat with more room.
 *   max_rows = h * w suffices for connected labels (every row between a connected label's first and last holds one of its
 *   pixels); it need not for scattered ones, whose rows in between count without holding a pixel.  max_rows <= 2^28.
 *   max_out = 0 is allowed (out may then be NULL).  Nothing but the outputs and the workspace is written, and the workspace may
 *   hold anything on entry.  Sides 1..16384; max_out, max_rows >= 0; workspace: unetdc_label_hull_workspace(h, w, max_out,
 *   max_rows) bytes (0 for arguments the call would refuse), 4-byte aligned.  UNETDC_EINVAL before any launch for a null pointer
 *   or a refused geometry.  Launches on the given stream only; no host wait, no allocation.  Integer atomic minima and maxima
 *   and sequential integer chains: bitwise reproducible. */
#define UNETDC_HULL_QUANTITIES 5
int64_t unetdc_label_hull_workspace(int h, int w, int max_out, int max_rows);
int unetdc_label_hull(const int32_t* label, int max_out, int h, int w, void* workspace, int64_t workspace_bytes, int64_t* out,
                      int32_t* out_rows, int max_rows, unetdc_stream_t s);


/* ---- ordered outlines per droplet: crack-following contours (outlines.hip; the definition is DESIGN.md section 27) -----------
 * unetdc_label_outlines: label ([h][w] int32: 0 = background, droplets 1..max_out; any label map: labels may touch and need not
 *   be connected; values below 1 or above max_out are skipped, and are "not k" to every droplet like the background).  Pixel
 *   (r, c) is the square [c, c + 1] x [r, r + 1]; corners are (x, y), x in 0..w, y in 0..h.  A crack of label k is a unit edge
 *   between a pixel of k and one that is not k (or the outside), directed with the k-pixel on its right on the screen (top: E,
 *   right: S, bottom: W, left: N); its id is (y_tail * (w + 1) + x_tail) * 4 + d, d = 0 E, 1 S, 2 W, 3 N.  Its successor, at
 *   its head facing d: ahead-right not k: turn right; else ahead-left not k: straight; else turn left.  The cracks of a label
 *   fall into cycles, its contours; a contour starts at its crack of smallest id, its vertices are the heads of the cracks whose
 *   successor has another direction, listed from the start's tail in walking order (nv >= 4, no three on a line), its length is
 *   its number of cracks and S2 = sum (x_tail * y_head - x_head * y_tail) is > 0 for an outer contour (clockwise on the screen),
 *   < 0 for a hole.  Contours are listed in ascending start id.
 *   -> out[UNETDC_OUTLINE_QUANTITIES][max_out] int64, row j of droplet k at out[j * max_out + k - 1]:
 *     0 E    number of cracks              3 nv   vertices over all its contours
 *     1 no   outer contours                4 F2   sum of S2 over the outer contours (twice the filled area)
 *     2 nh   hole contours                 5 S2   sum of S2 over all contours (twice the pixel count)
 *   A number without pixels keeps 0 in all six rows.
 *   -> contours[UNETDC_CONTOUR_FIELDS][max_contours] int64, field f of contour i at contours[f * max_contours + i]: label,
 *     first (index of its first vertex in vx / vy), nv, length, S2;  vx, vy[max_vertices] int32.
 *   -> needed[4] int32: the cracks, contours and vertices of the image, and too_long.
 *   Rooms: if needed[0] > max_cracks nothing else is computed: out is zero, needed[1..3] are 0 and only needed[0] means anything
 *   (it is cut at 2^31 - 1).  Otherwise out is always complete; contours and vertices are written where they fit their rooms
 *   (contour i if i < max_contours, a vertex if its index < max_vertices), and needed[1], needed[2] say how many there are.
 *   max_len bounds the length of a contour: the list ranking runs ceil(log2(max_len)) rounds.  If a contour is longer,
 *   needed[3] = 1, needed[1] = needed[2] = 0, out is zero and no contour or vertex is written: repeat with a larger max_len
 *   (max_len = needed[0] always suffices).  A 4-connected label of A pixels has at most 2 A + 2 cracks.
 *   max_out = 0 and rooms of 0 are allowed (out, contours, vx / vy may then be NULL).  Nothing but the outputs and the
 *   workspace is written, and the workspace may hold anything on entry.  Sides 1..16384, h * w < 2^30; max_out, max_len,
 *   max_contours, max_vertices >= 0; max_cracks 0..2^30; workspace: unetdc_label_outlines_workspace(h, w, max_out, max_cracks)
 *   bytes (0 for arguments the call would refuse), 8-byte aligned.  UNETDC_EINVAL before any launch for a null pointer, a
 *   refused geometry or a negative limit, UNETDC_EWORKSPACE for a workspace too small.  Launches on the given stream only; no
 *   host wait, no allocation.  Integer atomic adds and fixed-order scans: bitwise reproducible. */
#define UNETDC_OUTLINE_QUANTITIES 6
#define UNETDC_CONTOUR_FIELDS 5      /* label, first vertex, nv, length, S2 */
int64_t unetdc_label_outlines_workspace(int h, int w, int max_out, int max_cracks);
int unetdc_label_outlines(const int32_t* label, int max_out, int h, int w, int max_len, void* workspace, int64_t workspace_bytes,
                          int64_t* out, int64_t* contours, int max_contours, int32_t* vx, int32_t* vy, int max_vertices,
                          int max_cracks, int32_t* needed, unetdc_stream_t s);


/* ---- polygons back into a label map: exact even-odd fill (polyfill.hip; the definition is DESIGN.md section 28) --------------
 * unetdc_polygon_fill: verts ([n_verts][2] int32: x, y in sub-pixels, 256 per pixel, |v| <= 2^28), ring_first ([n_rings + 1]:
 *   ring j owns verts[ring_first[j] .. ring_first[j + 1])), poly_first_ring ([n_polys + 1]: polygon p owns the rings
 *   poly_first_ring[p] .. poly_first_ring[p + 1] - 1), poly_label ([n_polys], > 0; a polygon whose label is not is skipped), all
 *   on the device -> labels_out ([h][w] int32).  Pixel (r, c) is the square [c, c + 1] x [r, r + 1]; its centre is
 *   (X, Y) = (256 c + 128, 256 r + 128).  It is inside a polygon iff an odd number of the polygon's edges (x0, y0) -> (x1, y1),
 *   over all its rings, have (y0 <= Y) != (y1 <= Y) and, ordered so that y0 < y1, (X - x0)(y1 - y0) > (Y - y0)(x1 - x0):
 *   horizontal edges never count, a centre on an edge is not right of it, ring orientation does not matter.  labels_out is the
 *   largest label among the polygons that contain the pixel, 0 where none does; every pixel is written.  Vertices outside
 *   the image are legal.  Index ranges read from ring_first and poly_first_ring are clamped to the arrays.
 *   Limits: sides 1..16384, h * w < 2^30; n_verts 0..2^24; 3 n_rings <= n_verts; n_polys <= n_rings, n_polys <= 2^22; items
 *   (polygon, row) < 2^31, checked as n_polys * h < 2^31.  n_polys = 0 is allowed (verts and poly_label may then be NULL).
 *   workspace: unetdc_polygon_fill_workspace(h, w, n_polys, n_rings, n_verts) bytes (negative for arguments the call would
 *   refuse), 16-byte aligned; it may hold anything on entry.  UNETDC_EINVAL before any launch for a null pointer or a refused
 *   geometry, UNETDC_EWORKSPACE for a workspace too small.
 * unetdc_label_census: label ([h][w] int32) -> area[n_labels] int64: area[k - 1] = the pixels of value k, k = 1..n_labels (all
 *   n_labels entries are written; other values are not counted).  No workspace.
 * unetdc_label_relabel: label[i] = lut[label[i] - 1] for every pixel whose value lies in 1..n_lut, in place; lut int32 on the
 *   device.  Other pixels are not written.  No workspace.
 *   All three launch on the given stream only; no host wait, no allocation.  Integer atomic maxima and adds only: bitwise
 *   reproducible. */
int64_t unetdc_polygon_fill_workspace(int h, int w, int n_polys, int n_rings, int n_verts);
int unetdc_polygon_fill(const int32_t* verts, const int32_t* ring_first, const int32_t* poly_first_ring, const int32_t* poly_label,
                        int n_polys, int n_rings, int n_verts, int h, int w, int32_t* labels_out, void* workspace,
                        int64_t workspace_bytes, unetdc_stream_t s);
int unetdc_label_census(const int32_t* label, int h, int w, int n_labels, int64_t* area, unetdc_stream_t s);
int unetdc_label_relabel(int32_t* label, int h, int w, const int32_t* lut, int n_lut, unetdc_stream_t s);


/* ---- overlap table of two label maps (match.hip; the definition is DESIGN.md section 12) ------------------------------------
 * unetdc_label_overlap: label_a, label_b ([h][w] int32 each: 0 = background, objects 1..max_a and 1..max_b; any label maps,
 *   touching labels allowed) -> the triples (a, b, n) with n > 0 = the number of pixels that carry label a on the first map
 *   and label b on the second, in ascending order of (a, b): triple i at out_a[i], out_b[i], out_n[i].  Pixels whose label
 *   is below 1 or above max_a (max_b) on either side contribute nothing.
 *   *out_count = the number of triples; if there are more than max_pairs of them, *out_count = max_pairs + 1, the first
 *   max_pairs entries of the three arrays are unspecified and nothing beyond them is written.  max_pairs = h * w always
 *   suffices; max_pairs = 0 is allowed (the three arrays may then be NULL).  Nothing but the outputs and the workspace is
 *   written.  Sides 1..16384; max_a, max_b, max_pairs >= 0; workspace: unetdc_label_overlap_workspace(h, w, max_pairs) bytes
 *   (0 for arguments the call would refuse).  Integer atomics and a sort on unique keys: bitwise reproducible, order
 *   included. */
int64_t unetdc_label_overlap_workspace(int h, int w, int max_pairs);
int unetdc_label_overlap(const int32_t* label_a, int max_a, const int32_t* label_b, int max_b, int h, int w, void* workspace,
                         int64_t workspace_bytes, int32_t* out_count, int32_t* out_a, int32_t* out_b, int32_t* out_n,
                         int max_pairs, unetdc_stream_t s);


/* ---- droplet neighbourhoods of a label map (neighbors.hip; the definition is DESIGN.md section 20) --------------------------
 * unetdc_label_neighbors: label ([h][w] int32: 0 = background, droplets 1..max_label; any label map, touching labels allowed;
 *   values below 1 or above max_label are background) and radius (1..64 pixels) ->
 *     the contact pairs (a, b, d2), a < b, d2 = the smallest squared distance between a pixel of a and a pixel of b, all with
 *     d2 <= radius^2, in ascending order of (a, b): pair i at out_a[i], out_b[i], out_d2[i];
 *     per label k at index k - 1 of five int32 arrays of max_label entries: out_nn_label / out_nn_d2 (the contact with the
 *     smallest (d2, label); 0 and UNETDC_EDT_INF without one), out_degree (pairs that contain k), out_cluster (the smallest
 *     label of k's component of the contact graph), out_cluster_size (labels with a pixel in that component; 0 for a label
 *     without a pixel, which otherwise reads as an isolated one).
 *   *out_count = the number of pairs; if there are more than max_pairs of them, *out_count = max_pairs + 1, the first
 *   max_pairs entries of the three pair arrays and the five per-label arrays are unspecified and nothing beyond them is
 *   written: repeat with more room.  max_label * (max_label - 1) / 2 always suffices (h * w does not: a label can have many
 *   partners per pixel); the table holds at most 2^27 pairs.  max_pairs = 0 is allowed (the three pair arrays may then be
 *   NULL), and so is max_label = 0 (the five per-label arrays may then be NULL).  Nothing but the outputs and the workspace is
 *   written, and the workspace may hold anything on entry.  Sides 1..16384; max_label, max_pairs >= 0; workspace:
 *   unetdc_label_neighbors_workspace(h, w, max_label, max_pairs) bytes (0 for arguments the call would refuse), 8-byte
 *   aligned.  Launches on the given stream only; no host wait, no allocation.  Integer atomics and a sort on unique keys:
 *   bitwise reproducible, order included. */
int64_t unetdc_label_neighbors_workspace(int h, int w, int max_label, int max_pairs);
int unetdc_label_neighbors(const int32_t* label, int max_label, int h, int w, int radius, void* workspace,
                           int64_t workspace_bytes, int32_t* out_count, int32_t* out_a, int32_t* out_b, int32_t* out_d2,
                           int max_pairs, int32_t* out_nn_label, int32_t* out_nn_d2, int32_t* out_degree, int32_t* out_cluster,
                           int32_t* out_cluster_size, unetdc_stream_t s);


/* ---- droplets per cell: nearest-label territories and the per-cell table (cells.hip) -------------------
 * unetdc_label_nearest: label ([h][w] int32; the seed pixels are the pixels q with 1 <= label[q] <= max_label, any other value
 *   is not a seed; touching labels allowed), radius (0..32767 pixels, 0 = unbounded) -> for every pixel p, with (D, L) = the
 *   lexicographic minimum over the seed pixels q of (|p - q|^2, label[q]) -- the nearest seed pixel wins, among equidistant
 *   seed pixels the smallest label --: out_d2[p] = D, always the exact squared distance (below 2^30), and out_label[p] = L,
 *   or 0 where radius > 0 and D > radius^2.  A seed pixel gets its own label and 0.  Without any seed every out_label is 0
 *   and every out_d2 is UNETDC_EDT_INF.  out_label and out_d2 [h][w] int32, every pixel written; they and the workspace may
 *   hold anything on entry, and nothing else is written.  Sides 1..16384, max_label >= 0; workspace:
 *   unetdc_label_nearest_workspace(h, w) bytes (0 for a geometry the call would refuse), 4-byte aligned.  UNETDC_EINVAL before
 *   any launch for a null pointer or a refused argument, UNETDC_EWORKSPACE for a workspace too small.  Launches on the given
 *   stream only; no host wait, no allocation.  Integer minima defined per pixel: bitwise reproducible.
 * unetdc_cell_table: droplet_label and cell_label ([h][w] int32 each; values outside 1..max_droplet and 1..max_cell are
 *   background on their map), d2 ([h][w] int32, e.g. out_d2 of unetdc_label_nearest of the nuclei; may be NULL) ->
 *   out_droplet[UNETDC_CELL_DROPLET_QUANTITIES][max_droplet] int32, row j of droplet k at out_droplet[j * max_droplet + k - 1]:
 *     0 cell     the cell label that carries the most pixels of the droplet, the smallest label at ties; 0 if no pixel of
 *                the droplet lies on a cell
 *     1 n_in     pixels of the droplet on that cell
 *     2 n_cells  distinct cells the droplet has a pixel on
 *     3 n_out    pixels of the droplet on cell label 0
 *     4 area     pixels of the droplet
 *     5 min_d2   the minimum of d2 over the droplet's pixels; UNETDC_EDT_INF when d2 is NULL or the droplet has no pixel
 *   out_cell[UNETDC_CELL_QUANTITIES][max_cell] int64, row j of cell c at out_cell[j * max_cell + c - 1]:
 *     0 area        pixels of the cell
 *     1 n_border    pixels of the cell on the first or last row or column of the image
 *     2 fg_px       pixels of the cell that carry a droplet label (pixel-exact, independent of the assignment)
 *     3 n_droplets  droplets whose row 0 is this cell
 *     4 S_area      the sum of area over those droplets
 *     5 S_area2     the sum of area^2 over those droplets
 *     6 max_area    the largest area among those droplets, 0 without one
 *     7 nucleus_px  pixels of the cell with d2 == 0; 0 when d2 is NULL
 *   Every row is written for all max_droplet / max_cell entries.  *out_needed = the number of distinct (droplet, cell) pairs
 *   that share a pixel; if there are more than max_pairs of them, *out_needed = max_pairs + 1 and all other outputs are
 *   unspecified: repeat with more room (h * w always suffices).  max_droplet = 0 and max_cell = 0 are allowed (the output of
 *   that side may then be NULL).  Nothing but the outputs and the workspace is written; both may hold anything on entry.
 *   Sides 1..16384; max_droplet, max_cell, max_pairs >= 0; workspace: unetdc_cell_table_workspace(h, w, max_droplet,
 *   max_cell, max_pairs) bytes (0 for arguments the call would refuse; max_cell does not enter it), 8-byte aligned like
 *   out_cell.  Launches on the given stream only; no host wait, no allocation.  Integer atomics, and an argmax on unique
 *   keys: bitwise reproducible. */
#define UNETDC_CELL_DROPLET_QUANTITIES 6
#define UNETDC_CELL_QUANTITIES 8
int64_t unetdc_label_nearest_workspace(int h, int w);
int unetdc_label_nearest(const int32_t* label, int max_label, int h, int w, int radius, void* workspace, int64_t workspace_bytes,
                         int32_t* out_label, int32_t* out_d2, unetdc_stream_t s);
int64_t unetdc_cell_table_workspace(int h, int w, int max_droplet, int max_cell, int max_pairs);
int unetdc_cell_table(const int32_t* droplet_label, int max_droplet, const int32_t* cell_label, int max_cell, const int32_t* d2,
                      int h, int w, void* workspace, int64_t workspace_bytes, int32_t* out_needed, int max_pairs,
                      int32_t* out_droplet, int64_t* out_cell, unetdc_stream_t s);


/* ---- Ripley's K of the droplet centroids with simulated patterns (spatial.hip; the definition is DESIGN.md section 26) --------
 * unetdc_droplet_points: the droplet table of unetdc_ccl_stats (*count droplets: area, sum of rows, sum of columns; device
 *   memory) -> the centroid pixels y = (2 sum_y + area) div (2 area), x likewise, of the droplets whose pixel lies in the
 *   window (uint8 [h][w], nonzero = inside; NULL: every pixel), in table order: out_py / out_px (int32 [max_points]).
 *   out_info (int32 [4]): N (the points written), n_dropped, A (the pixels of the window) and a flags word; bit 0 of the
 *   flags: *count exceeds max_points, the other outputs are then unspecified and nothing beyond max_points entries is
 *   written: repeat with more room.  Sides 1..16384, max_points 1..2^20.
 * unetdc_ripley_counts: N = *n_points points (py, px: int32, inside the image and the window; N is cut to max_points) -> for
 *   r = 0..rmax and the point sets 0 (the given points) and s + 1 (simulation s of n_sim: N pixels of the window drawn with
 *   replacement by a counter hash of (seed, s, k)):
 *     out_n [(1 + n_sim)][rmax + 1] int32: the points whose distance to the border of the window and of the image exceeds r;
 *     out_pairs, out_pairs_all (int64, same shape): the ordered pairs (i, j), i != j, at most r apart (the distance rounded
 *     up to an integer), out_pairs only those whose i counts in out_n at r.
 *   The simulation rows are zero without a point or without a window pixel.  rmax 1..256, n_sim 0..999, max_points 1..2^20,
 *   sides 1..16384; workspace: unetdc_ripley_workspace(h, w, max_points, rmax, n_sim) bytes (0 for arguments the call would
 *   refuse), 8-byte aligned; it may hold anything on entry.  Nothing but the outputs and the workspace is written.
 * Both launch on the given stream only: no host wait, no allocation.  Integer work and integer atomics: bitwise
 * reproducible. */
int64_t unetdc_ripley_workspace(int h, int w, int max_points, int rmax, int n_sim);
int unetdc_droplet_points(const int32_t* count, const int32_t* area, const int64_t* sum_y, const int64_t* sum_x, int max_points,
                          const uint8_t* window, int h, int w, int32_t* out_py, int32_t* out_px, int32_t* out_info,
                          unetdc_stream_t s);
int unetdc_ripley_counts(const int32_t* py, const int32_t* px, const int32_t* n_points, int max_points, const uint8_t* window,
                         int h, int w, int rmax, int n_sim, uint32_t seed, void* workspace, int64_t workspace_bytes,
                         int32_t* out_n, int64_t* out_pairs, int64_t* out_pairs_all, unetdc_stream_t s);


/* ---- surface distances between two label maps (boundary.hip; the definition is DESIGN.md section 21) -----------------------
 * unetdc_boundary_distances: label_a (the prediction), label_b (the annotation): [h][w] int32 label maps, objects 1..max_a and
 *   1..max_b; a value below 1 or above the maximum reads as 0.  A binary mask is the label map with max = 1.
 *   A pixel is a BOUNDARY pixel of its map when it carries a label (after that rule) and one of its 4-neighbours lies outside the
 *   image or carries another value (after that rule): the cut between two touching objects is boundary, and so is the frame.
 *   For every boundary pixel p of one map, d2(p) = the smallest squared Euclidean distance to a boundary pixel of the other map
 *   (of ANY object of it, not of a matched partner): an exact integer below 2^29, UNETDC_EDT_INF when the other map has none.
 *     hist (DEVICE, [2][radius^2 + 2] int64, 8-byte aligned): hist[0][min(d2(p), radius^2 + 1)] += 1 for every boundary pixel
 *       of label_a, hist[1][.] likewise for label_b; bin radius^2 + 1 is "far".  The call ADDS; the caller zeroes hist once and
 *       may pool any number of images in it.
 *     dmax (DEVICE, [2] int32): dmax[dir] = max(dmax[dir], the largest d2 of that direction), unclamped; the caller
 *       initialises it to -1.
 *     out_a (nullable, [3][max_a] int64, 8-byte aligned): for object k at index k - 1, row 0 = its boundary pixels, row 1 = the
 *       largest d2 among them (-1 without one), row 2 = the sum of their d2 (unclamped).  Every entry is initialised by the
 *       call.  out_b ([3][max_b]): the same for label_b.  NULL: no table for that side.
 *   Sides 1..16384, radius 1..64, max_a, max_b >= 0; anything else, a null label map / workspace / hist / dmax or a misaligned
 *   pointer returns UNETDC_EINVAL before the first launch, a workspace below unetdc_boundary_distances_workspace(h, w) bytes
 *   (10 per pixel + 64; 0 for a geometry the call refuses; 4-byte aligned) UNETDC_EWORKSPACE.  Nothing but hist, dmax, the two
 *   tables and the workspace is written, and the workspace may hold anything on entry.  Launches on the given stream only; no
 *   host wait, no allocation.  Integer atomics only: the result depends on no order, two runs are bitwise equal. */
int64_t unetdc_boundary_distances_workspace(int h, int w);
int unetdc_boundary_distances(const int32_t* label_a, int max_a, const int32_t* label_b, int max_b, int h, int w, int radius,
                              void* workspace, int64_t workspace_bytes, int64_t* hist, int32_t* dmax, int64_t* out_a,
                              int64_t* out_b, unetdc_stream_t s);


/* ---- cleaning a mask before the droplet stages (clean.hip; the definition is DESIGN.md section 13) --------------------------
 * unetdc_mask_clean: strong and weak ([h][w] uint8, nonzero = 1; weak may be NULL) -> out_mask ([h][w] uint8 in {0,1}):
 *     hysteresis  (weak given) M = the union of the 4-connected components of weak that contain a pixel where strong and weak
 *                 are both 1; a strong pixel outside weak is ignored.  Without weak, M = strong.
 *     holes       (max_hole_area != 0) a hole is a 4-connected component of the background of M without a pixel on the first
 *                 or last row or column; every hole of at most max_hole_area pixels (any size when max_hole_area < 0) is
 *                 set to 1 (= scipy.ndimage.binary_fill_holes when there is no limit).
 *   out_counts (DEVICE, 4 x int32, may be NULL): pixels of M not in strong, holes filled, pixels filled, holes left open
 *   because of their size (the last three are 0 when max_hole_area == 0).
 *   With weak == NULL and max_hole_area == 0 the call copies strong to out_mask.
 *   Aliasing: out_mask may BE strong or weak (the same pointer: the call then works in place); an out_mask that overlaps
 *   either only partly, and a workspace or out_counts that overlaps any other argument, return UNETDC_EINVAL.  strong and weak
 *   may overlap each other in any way.
 *   Sides 1..16384; workspace: unetdc_mask_clean_workspace(h, w) bytes (8 per pixel + 64; 0 for a side out of range), 4-byte
 *   aligned.  A bad geometry, a null strong / out_mask / workspace and a workspace that is too small return UNETDC_EINVAL
 *   before the first launch.  Launches on the given stream only; no host wait, no allocation.  Flags, integer atomics and a
 *   union-find: the outputs depend on no order, two runs are bitwise equal. */
int64_t unetdc_mask_clean_workspace(int h, int w);
int unetdc_mask_clean(const uint8_t* strong, const uint8_t* weak, int h, int w, int max_hole_area, void* workspace,
                      int64_t workspace_bytes, uint8_t* out_mask, int32_t* out_counts, unetdc_stream_t s);


/* ---- difference map against an annotation and its regions (diffmap.hip; the definition is DESIGN.md section 25) --------------
 * pred, gt ([h][w] uint8 each, nonzero = 1) give the class plane c = pred | gt << 1 and its colours, the reference's:
 *     0 black (0, 0, 0): neither (TN)        1 green (0, 255, 0): only predicted (FP)
 *     2 red (255, 0, 0): only annotated (FN) 3 yellow (255, 255, 0): both (TP)
 * unetdc_diff_regions: a REGION is a maximal 8-connected set of pixels of equal c; all four classes count, black included.
 *     out_image (DEVICE, int64 [12], 8-byte aligned): pixels[4] (the pixel count of each class), regions[4] (every region of
 *       each class), kept[4] (the regions of each class with area >= min_area).
 *     The table: one row per region of class 1..3 with area >= min_area, in raster order of the region's first pixel, the
 *       classes interleaved: row i at out_class[i], out_area[i] (int32), out_sumy[i], out_sumx[i] (int64: the sums of the row
 *       and column coordinates of its pixels), out_neighbors[i] (int32: bit k is set when some pixel of the region has an
 *       8-neighbour of class k != class; the image border sets no bit).
 *     *out_count = the number of rows that exist; it may exceed max_out, rows past max_out are not written.  max_out = 0 is
 *       allowed (the five table arrays may then be NULL).
 *   Sides 1..16384 with h * w < 2^30, min_area >= 1, max_out >= 0; anything else, a null pred / gt / workspace / out_image /
 *   out_count, a null table with max_out > 0 or a misaligned pointer (workspace, out_image, out_sumy, out_sumx: 8 bytes; the
 *   int32 outputs: 4) returns UNETDC_EINVAL before the first launch, a workspace below unetdc_diff_regions_workspace(h, w)
 *   bytes UNETDC_EWORKSPACE.  The query answers 29 n + 4 ceil(n / 1024) + 128 bytes for n = h * w pixels (two int64 and three
 *   int32 planes, one word per 1024 pixels and 16 more, one byte plane, 64 spare bytes) and 0 for a geometry the call refuses.
 *   pred and gt are only read; nothing but the outputs and the workspace is written, and the workspace may hold anything on
 *   entry.  Launches on the given stream only; no host wait, no allocation.  Integer atomics and a union-find whose root is the
 *   region's smallest linear index: the outputs depend on no order, two runs are bitwise equal.
 * unetdc_diff_paint: out_diff ([h][w][3] uint8, nullable): the colour of c at every pixel.  out_overlay ([h][w][3] uint8,
 *   nullable): rgb ([h][w][3] uint8, required with out_overlay, else ignored and nullable) with every pixel of c != 0 replaced
 *   by its colour.  At least one output must be given; no output may overlap an input or the other output.  Same limits on the
 *   sides; UNETDC_EINVAL before the launch otherwise.  No alignment is required: planes that are all 4-byte aligned move as
 *   whole dwords, any other set byte by byte, with equal results.  No workspace, no atomics, one launch on the given stream. */
int64_t unetdc_diff_regions_workspace(int h, int w);
int unetdc_diff_regions(const uint8_t* pred, const uint8_t* gt, int h, int w, int min_area, void* workspace,
                        int64_t workspace_bytes, int64_t* out_image, int32_t* out_count, int32_t* out_class, int32_t* out_area,
                        int64_t* out_sumy, int64_t* out_sumx, int32_t* out_neighbors, int max_out, unetdc_stream_t s);
int unetdc_diff_paint(const uint8_t* pred, const uint8_t* gt, const uint8_t* rgb, int h, int w, uint8_t* out_diff,
                      uint8_t* out_overlay, unetdc_stream_t s);


/* ---- threshold sweep against an annotation (sweep.hip; the definition is DESIGN.md section 14) ------------------------------
 * unetdc_thresh_sweep: probs ([n][ph][pw] fp32), gt ([n][oh][ow] uint8, nonzero = annotated), n >= 1 images of one geometry,
 *   k in 1..1024 thresholds t_j = (float)j / (float)k, j = 0..k-1 (one fp32 division each).
 *   mask_j = what unetdc_mask_from_probs (xofs, xcoef, yofs, ycoef all NULL: nearest rule) or unetdc_mask_from_probs_linear (all
 *   four given: the tables of that call) writes for thresh = t_j: strict > in fp32, a NaN probability is never set.  Both rules
 *   are monotone in the threshold, so every output pixel has one level = the number of j with mask_j = 1, in 0..k, and
 *   mask_j = 1 exactly when j < level.
 *   hist (DEVICE, [2][k + 1] int64, 8-byte aligned): hist[g][l] += the number of pixels with (gt != 0) == g and level l.  The
 *   call ADDS; the caller zeroes hist once and may pool any number of calls in it.  Then, for every j,
 *   tp_j = sum over l > j of hist[1][l], fp_j = the same sum over hist[0], fn_j and tn_j the rest of each row.
 *   Nothing but hist is written; no workspace, no host wait, no allocation; launches on the given stream only.
 *   UNETDC_EINVAL before any launch: a null probs / gt / hist, k outside 1..1024, a side outside 1..16384, n < 1, some but not
 *   all of the four tables.  Integer atomics only: the result depends on no order, two runs are bitwise equal. */
int unetdc_thresh_sweep(const float* probs, int n, int ph, int pw, const uint8_t* gt, int oh, int ow, const int32_t* xofs,
                        const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef, int k, int64_t* hist,
                        unetdc_stream_t s);


/* ---- tiled inference at native resolution (tile.hip; the definition is DESIGN.md section 15, utils/tiling.py) ------------------
 * A plan is two ascending origin lists yo[ny], xo[nx] (DEVICE int32 arrays; utils/tiling.py:tile_plan builds them): tile number
 * ty * nx + tx has its corner at (yo[ty], xo[tx]) and t x t pixels; t is a multiple of 16 in 16..4096 (the plan itself asks for
 * at least 32); at most 1024 tiles per axis; image sides 1..16384.
 * unetdc_tile_gather_u8_to_chw_f32: src_hwc ([h][w][channels] uint8, channels 1..4) -> tiles ([count][channels][t][t] fp32,
 *   16-byte aligned) for the tile numbers t0 .. t0 + count - 1: float(v) / 255.0f (one IEEE division, the expression of
 *   unetdc_resize_linear_u8_to_chw_f32) of the pixel at (yo[ty] + y, xo[tx] + x); a coordinate outside the image folds back by
 *   reflect-101 with as many reflections as needed (period 2 (side - 1); a side of 1 maps to 0), so that every read lies inside
 *   src whatever the origin arrays hold.
 * unetdc_tile_blend_f32: tile_probs ([ny * nx][t][t] fp32) -> out ([h][w] fp32):
 *     out[y][x] = sum(wy wx p) / sum(wy wx) over the tiles with 0 <= y - yo[ty] < t and 0 <= x - xo[tx] < t, in ascending tile
 *     number, w(i) = min(i + 1, t - i, max(overlap, 1)) at the tile-local index i (0 <= overlap <= t / 2); both sums in fp32,
 *     product and sum rounded separately, one IEEE division.  Only those elements of tile_probs are read: never the folded
 *     part of a tile of an image smaller than t.  Every pixel of out is written; a pixel that no tile covers (origins that are
 *     not a plan of h x w) gets NaN.
 * Both: nothing but the output is written; no workspace, no allocation, no host wait, no atomics; launches on the given stream
 * only; two runs are bitwise equal.  UNETDC_EINVAL before any launch: a null pointer, a side, channel count, tile size, overlap
 * or tile count outside the limits above, t0 < 0, count < 1 or t0 + count > ny * nx, a misaligned tile buffer. */
int unetdc_tile_gather_u8_to_chw_f32(const uint8_t* src_hwc, int h, int w, int channels, float* tiles, int t, const int32_t* yo,
                                     int ny, const int32_t* xo, int nx, int t0, int count, unetdc_stream_t s);
int unetdc_tile_blend_f32(const float* tile_probs, int t, int overlap, const int32_t* yo, int ny, const int32_t* xo, int nx,
                          float* out, int h, int w, unetdc_stream_t s);


/* ---- test-time augmentation over the dihedral group (tta.hip; the definition is DESIGN.md section 17, utils/tta.py) -----------
 * Variant v in 0..7 of a square plane P [s][s]: hflip = v & 4, k = v & 3, variant(P) = np.rot90(P[:, ::-1] if hflip else P, k)
 * (flip first, then k counter-clockwise quarter turns: the order of unetdc_augment_gather).  nvar in {1, 2, 4, 8} stands for the
 * ordered variant lists [0], [0, 4], [0, 4, 2, 6], [0, 1, ..., 7].  s is a multiple of 16 in 16..4096, n in 1..4096, c in 1..4.
 * unetdc_dihedral_expand_f32: x ([n][c][s][s] fp32) -> out ([n * nvar][c][s][s] fp32): item b * nvar + i is variant list[i] of
 *   image b, every channel alike.  A permutation: bit-exact.
 * unetdc_dihedral_mean_f32: p ([n * nvar][s][s] fp32) -> out ([n][s][s] fp32): per pixel acc = q_0, then acc = acc + q_i in list
 *   order, every add rounded in fp32, then one IEEE division by float(nvar); q_i is item b * nvar + i mapped back through the
 *   inverse of variant list[i].  nvar == 1 copies the input bits.
 * unetdc_dihedral_mean_env_f32: the same mean into out_mean, bit for bit, and from the same pass out_lo / out_hi ([n][s][s] fp32
 *   each): the minimum / maximum of the q_i (fminf / fmaxf: numpy's minimum / maximum on inputs without a NaN).  lo <= hi holds;
 *   lo <= mean <= hi does not (the rounded fp32 mean of equal values may miss them).  Every buffer 16-byte aligned; no output
 *   may overlap the input or another output.
 * All: nothing but the outputs is written; no workspace, no allocation, no host wait, no atomics; launches on the given stream only;
 * two runs are bitwise equal.  UNETDC_EINVAL before any launch: a null pointer, s, n, c or nvar outside the limits above, a
 * buffer that is not 16-byte aligned, out overlapping the input. */
int unetdc_dihedral_expand_f32(const float* x, int n, int c, int s, int nvar, float* out, unetdc_stream_t stream);
int unetdc_dihedral_mean_f32(const float* p, int n, int s, int nvar, float* out, unetdc_stream_t stream);
int unetdc_dihedral_mean_env_f32(const float* p, int n, int s, int nvar, float* out_mean, float* out_lo, float* out_hi,
                                 unetdc_stream_t stream);

/* ---- deep (16-bit) images -> the 8-bit image the flow takes (window.hip; the definition is DESIGN.md section 29,
 * utils/intensity_window.py) -------------------------------------------------------------------------------------------------
 * src is uint16, interleaved [h][w][c], c in 1..4, sides 1..16384, h * w < 2^30; n = h * w values per channel.
 * unetdc_u16_ranks: nq in 1..8 requests ppm[j] in 0..1000000 (HOST array, read before the call returns; any order, repeats
 *   allowed).  k_j = max(1, ceil(ppm[j] * n / 10^6)) in int64; out_value[ch][j] = the k_j-th smallest value of channel ch
 *   (nearest rank: 0 asks for the minimum, 10^6 for the maximum), out_below = the number of values < value, out_equal the number
 *   == value (DEVICE int32 [c][nq] each, 4-byte aligned).  The workspace (unetdc_u16_ranks_workspace bytes; 0 for a refused
 *   geometry) may hold anything: the call zeroes the counters it uses.
 * unetdc_window_u16_to_u8: levels (DEVICE int32 [c][2], lo then hi per channel, clamped to 0..65535 when read): d = hi - lo;
 *   for d > 0: t = min(max(v, lo), hi) - lo and dst = (510 t + d) / (2 d) by integer division (255 t / d rounded half up); for
 *   d <= 0: dst = 0.  dst is uint8 [h][w][dc], dc == c, or dc == 3 with c == 1 (the grey value three times).
 * unetdc_planes_max_u16: src ([planes][h][w] uint16, planes in 1..256) -> dst ([h][w] uint16): the maximum over the planes.
 * All: nothing but the outputs and the workspace is written; no allocation, no host wait, no copy to the host; launches on the
 *   given stream only; integer atomics only, so two runs are bitwise equal.  Before any launch: UNETDC_EINVAL for a null
 *   pointer, a geometry, channel, rank or plane count outside the limits above, a request outside 0..10^6; UNETDC_EWORKSPACE for
 *   a workspace smaller than the query's answer; then UNETDC_EINVAL for an image or a workspace that is not 16-byte aligned. */
int64_t unetdc_u16_ranks_workspace(int h, int w, int c, int nq);
int unetdc_u16_ranks(const uint16_t* src, int h, int w, int c, const int32_t* ppm, int nq, void* workspace, int64_t workspace_bytes,
                     int32_t* out_value, int32_t* out_below, int32_t* out_equal, unetdc_stream_t s);
int unetdc_window_u16_to_u8(const uint16_t* src, int h, int w, int c, const int32_t* levels, uint8_t* dst, int dc,
                            unetdc_stream_t s);
int unetdc_planes_max_u16(const uint16_t* src, int planes, int h, int w, uint16_t* dst, unetdc_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* UNETDC_HIP_H */
