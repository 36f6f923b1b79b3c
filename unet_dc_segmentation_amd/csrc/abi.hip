// extern "C" entry points of libunetdc_hip.so (declared in include/unetdc_hip.h).
// Thin argument validation + geometry setup; the kernels live in the other translation units.
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include <mutex>
#include <vector>

#include "../../include/unetdc_hip.h"
#include "kernels.h"

namespace unetdc {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static thread_local char g_kernel[128] = "";
void note_kernel(const char* name) { snprintf(g_kernel, sizeof(g_kernel), "%s", name); }

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return UNETDC_ELAUNCH;
  }
  return UNETDC_OK;
}

int ensure_dynamic_lds(const void* fn, int bytes, const char* name) {
  struct Entry { const void* fn; int dev; int bytes; };
  static std::mutex mu;
  static std::vector<Entry> memo;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> lock(mu);
  Entry* hit = nullptr;
  for (Entry& e : memo)
    if (e.fn == fn && e.dev == dev) { hit = &e; break; }
  if (hit && hit->bytes >= bytes) return UNETDC_OK;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) {
    set_error("hipFuncSetAttribute(%s, %d bytes of LDS) failed on device %d: %s", name, bytes, dev, hipGetErrorString(e));
    return UNETDC_ELAUNCH;
  }
  if (hit) hit->bytes = bytes;
  else memo.push_back(Entry{fn, dev, bytes});
  return UNETDC_OK;
}

static void taps3x3(int d, int* offy, int* offx) {
  for (int t = 0; t < 9; ++t) {
    offy[t] = (t / 3 - 1) * d;
    offx[t] = (t % 3 - 1) * d;
  }
}
static void taps2x2(int* offy, int* offx) {
  for (int t = 0; t < 4; ++t) { offy[t] = t >> 1; offx[t] = t & 1; }
}

// The implicit GEMM of a dilated 3 x 3 convolution over n x h x w with cin input and cout output channels (the input
// gradient passes them swapped), and of the input gradient of ConvTranspose2d(2, 2, stride 2): four taps of stride 2.
static IgemmParams conv3x3_igemm(int n, int h, int w, int cin, int cout, int ldx, int ldo, int d) {
  IgemmParams p{};
  p.M = n * h * w; p.Ho = h; p.Wo = w; p.Hi = h; p.Wi = w; p.Cin = cin; p.Cout = cout; p.ldx = ldx; p.ldo = ldo;
  p.ntaps = 9; p.stride = 1;
  taps3x3(d, p.offy, p.offx);
  return p;
}
static IgemmParams convT2x2_dgrad_igemm(int n, int h, int w, int cin, int cout, int lddup, int lddx) {
  IgemmParams p{};
  p.M = n * h * w; p.Ho = h; p.Wo = w; p.Hi = 2 * h; p.Wi = 2 * w; p.Cin = cout; p.Cout = cin; p.ldx = lddup;
  p.ldo = lddx; p.ntaps = 4; p.stride = 2;
  taps2x2(p.offy, p.offx);
  return p;
}

// The weight gradient of the same dilated 3 x 3 convolution: a = dy [P][lddy], b = x [P][ldx], out [cout][cin][9].
static WgradParams conv3x3_wgrad(int n, int h, int w, int cin, int cout, int ldx, int lddy, int d) {
  WgradParams p{};
  p.N = n; p.H = h; p.W = w; p.Hb = h; p.Wb = w; p.CI = cout; p.CJ = cin;
  p.lda = lddy; p.ldb = ldx; p.ntaps = 9; p.stride = 1;
  taps3x3(d, p.offy, p.offx);
  return p;
}

// One filler per parameter block of the BatchNorm backward and the head.
static BnBwdParams bn_bwd_params(const void* dskip, int ldskip, const void* dpool, int ldpool, const void* y, int ldy,
                                 const float* scale, const float* shift, const float* mean, const float* rstd, void* dy, int lddy,
                                 int n, int h, int w, int c) {
  BnBwdParams p{};
  p.dskip = dskip; p.dpool = dpool; p.y = y; p.dy = dy; p.scale = scale; p.shift = shift; p.mean = mean; p.rstd = rstd;
  p.N = n; p.H = h; p.W = w; p.C = c; p.lds = ldskip; p.ldp = ldpool; p.ldy = ldy; p.lddy = lddy;
  return p;
}
static HeadParams head_params(const void* a, int lda, const float* w, const float* probs, const float* dprobs, void* da, int ldda,
                              int n, int h, int wd, int c, int oc) {          // forward: dprobs, da null
  HeadParams p{};
  p.a = a; p.w = w; p.probs = const_cast<float*>(probs); p.dprobs = dprobs; p.da = da;
  p.N = n; p.H = h; p.W = wd; p.C = c; p.OC = oc; p.lda = lda; p.ldda = ldda;
  return p;
}

// Capability queries plan a call without launching it; a non-null in_scale only says "normalise the input on load".
static const float g_plan_marker = 0.f;

}  // namespace unetdc

using namespace unetdc;

#define GEOM_CHECK(n, h, w)                                                                          \
  UNETDC_REQUIRE((n) > 0 && (h) > 0 && (w) > 0, "bad geometry n=%d h=%d w=%d", (int)(n), (int)(h), (int)(w))

extern "C" {

int unetdc_version(void) { return UNETDC_ABI_VERSION; }
const char* unetdc_last_error(void) { return g_err; }
const char* unetdc_last_kernel(void) { return g_kernel; }

int unetdc_pack_conv3x3(const float* w, void* w_fwd, void* w_dgrad, int cout, int cin, int dtype, unetdc_stream_t s) {
  return launch_pack_conv3x3(w, w_fwd, w_dgrad, cout, cin, dtype, (hipStream_t)s);
}
int unetdc_pack_convT2x2(const float* w, void* w_fwd, void* w_dgrad, int cin, int cout, int dtype, unetdc_stream_t s) {
  return launch_pack_convT2x2(w, w_fwd, w_dgrad, cin, cout, dtype, (hipStream_t)s);
}

int unetdc_pack_many(const unetdc_pack_desc* table_dev, int n, int64_t total_tiles, int dtype, unetdc_stream_t s) {
  static_assert(sizeof(unetdc_pack_desc) == 48, "unetdc_pack_desc layout");
  return launch_pack_many(table_dev, n, (long)total_tiles, dtype, (hipStream_t)s);
}

int unetdc_adam_step(const unetdc_adam_desc* table_dev, int n, int64_t total_blocks, const float* flat_grad, double lr,
                     double beta1, double beta2, double eps, int64_t step, double grad_scale, int dtype, unetdc_stream_t s) {
  static_assert(sizeof(unetdc_adam_desc) == 80, "unetdc_adam_desc layout");
  return launch_adam_step(table_dev, n, (long)total_blocks, flat_grad, lr, beta1, beta2, eps, (long)step, grad_scale, dtype,
                          (hipStream_t)s);
}

int64_t unetdc_grad_norm_workspace(int64_t n) { return grad_norm_workspace_bytes((long)n); }

int unetdc_grad_norm(const float* flat_grad, int64_t n, double grad_scale, double max_norm, unetdc_step_ctl* ctl_dev,
                     void* workspace, int64_t workspace_bytes, unetdc_stream_t s) {
  static_assert(sizeof(unetdc_step_ctl) == 56 && offsetof(unetdc_step_ctl, gscale_eff) == 16 &&
                offsetof(unetdc_step_ctl, steps) == 24, "unetdc_step_ctl layout (mirrored by unet_dc_segmentation_amd/optim.py)");
  return launch_grad_norm(flat_grad, (long)n, grad_scale, max_norm, ctl_dev, workspace, (long)workspace_bytes, (hipStream_t)s);
}

int unetdc_adam_step_ex(const unetdc_adam_desc* table_dev, int n, int64_t total_blocks, const float* flat_grad, double lr,
                        double beta1, double beta2, double eps, int64_t step, double grad_scale, int dtype,
                        const unetdc_step_ctl* ctl_dev, double weight_decay, float* ema_base, const float* m_base,
                        double ema_decay, unetdc_stream_t s) {
  return launch_adam_step_ex(table_dev, n, (long)total_blocks, flat_grad, lr, beta1, beta2, eps, (long)step, grad_scale, dtype,
                             ctl_dev, weight_decay, ema_base, m_base, ema_decay, (hipStream_t)s);
}

int unetdc_conv3x3_stats_rows(int64_t npixels, int cout) { return igemm_mblocks((long)npixels, cout); }

int unetdc_conv3x3_fwd(const void* x, int ldx, const void* w_fwd, const float* bias, const float* scale,
                       const float* shift, void* y, int ldy, float* stats_part, int* stats_rows, int n, int h, int w,
                       int cin, int cout, int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(dilation >= 1, "conv3x3_fwd: dilation must be >= 1");
  UNETDC_REQUIRE(ldx >= cin && ldy >= cout, "conv3x3_fwd: ld smaller than channel count");
  IgemmParams p = conv3x3_igemm(n, h, w, cin, cout, ldx, ldy, dilation);
  p.x = x; p.w = w_fwd; p.out = y; p.bias = bias; p.scale = scale; p.shift = shift; p.stats = stats_part;
  p.mode = scale ? MODE_AFFINE_RELU : (stats_part ? MODE_STATS : MODE_STORE);
  const int rc = launch_igemm(p, dtype, (hipStream_t)s);
  if (rc == UNETDC_OK && p.mode == MODE_STATS && stats_rows) *stats_rows = p.mblocks;   // rows that carry data (the rest are zeros)
  return rc;
}

// forward conv fed from the RAW output of the stage in front of it: that stage's BatchNorm + ReLU is applied per staged patch
int unetdc_conv3x3_bnin_supported(int n, int h, int w, int cin, int cout, int dilation, int dtype) {
  if (n <= 0 || h <= 0 || w <= 0 || dilation < 1) return 0;
  IgemmParams p = conv3x3_igemm(n, h, w, cin, cout, cin, cout, dilation);
  p.mode = MODE_STATS; p.in_scale = &g_plan_marker;
  const IgemmPlan pl = plan_igemm(p, dtype);
  if (pl.route != IGEMM_LATTICE) return 0;
  if (pl.writes_act) return 2;       // forward stores the activation: any weight-gradient kernel follows
  WgradParams g = conv3x3_wgrad(n, h, w, cin, cout, cin, cout, dilation);
  g.in_scale = &g_plan_marker;
  return plan_wgrad(g, dtype).route != WGRAD_UNSUPPORTED ? 1 : 0;
}

int unetdc_conv3x3_fwd_bnin(const void* x_raw, int ldx, const float* in_scale, const float* in_shift, const void* w_fwd,
                            const float* bias, void* y, int ldy, float* stats_part, int* stats_rows, void* act_out, int ldact,
                            int n, int h, int w, int cin, int cout, int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(dilation >= 1 && ldx >= cin && ldy >= cout, "conv3x3_fwd_bnin: bad dilation/ld");
  UNETDC_REQUIRE(in_scale && in_shift && stats_part, "conv3x3_fwd_bnin: null pointer");
  UNETDC_REQUIRE(act_out == nullptr || (ldact >= cin && ldact % 8 == 0 && (int64_t)n * h * w * ldact * 2 < (1LL << 32)),
                 "conv3x3_fwd_bnin: bad activation ld (or an activation tensor of 4 GiB and more)");
  IgemmParams p = conv3x3_igemm(n, h, w, cin, cout, ldx, ldy, dilation);
  p.act_out = act_out; p.ld_act = ldact;
  p.x = x_raw; p.w = w_fwd; p.out = y; p.bias = bias; p.stats = stats_part; p.in_scale = in_scale; p.in_shift = in_shift;
  p.mode = MODE_STATS;
  const IgemmPlan pl = plan_igemm(p, dtype);
  if (pl.route != IGEMM_LATTICE || (act_out && !pl.writes_act)) {
    set_error("conv3x3_fwd_bnin: shape not supported by the input-normalising kernel%s (ask unetdc_conv3x3_bnin_supported)",
              act_out ? " that also stores the activation" : "");
    return UNETDC_EUNSUPPORTED;
  }
  const int rc = launch_igemm(p, dtype, (hipStream_t)s);
  if (rc == UNETDC_OK && stats_rows) *stats_rows = p.mblocks;
  return rc;
}

int unetdc_conv3x3_wgrad_bnin(const void* x_raw, int ldx, const float* in_scale, const float* in_shift, const void* dy,
                              int lddy, float* dw, void* workspace, int64_t workspace_bytes, int n, int h, int w, int cin,
                              int cout, int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(dilation >= 1 && in_scale && in_shift, "conv3x3_wgrad_bnin: bad arguments");
  WgradParams p = conv3x3_wgrad(n, h, w, cin, cout, ldx, lddy, dilation);
  p.a = dy; p.b = x_raw; p.in_scale = in_scale; p.in_shift = in_shift;
  return launch_wgrad(p, dw, workspace, (long)workspace_bytes, dtype, (hipStream_t)s);
}

int unetdc_conv3x3_dgrad(const void* dy, int lddy, const void* w_dgrad, void* dx, int lddx, int n, int h, int w,
                         int cin, int cout, int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(dilation >= 1, "conv3x3_dgrad: dilation must be >= 1");
  UNETDC_REQUIRE(lddy >= cout && lddx >= cin, "conv3x3_dgrad: ld smaller than channel count");
  IgemmParams p = conv3x3_igemm(n, h, w, cout, cin, lddy, lddx, dilation);
  p.x = dy; p.w = w_dgrad; p.out = dx; p.mode = MODE_STORE;
  return launch_igemm(p, dtype, (hipStream_t)s);
}

// dgrad whose epilogue also sums the stored gradient per channel: colsum[c] = sum_pixels dx[:, c0 + c]
int64_t unetdc_conv3x3_dgrad_colsum_workspace(int n, int h, int w, int cin) {
  return partial_floats(igemm_mblocks((long)n * h * w, cin), 2L * cin) * 4;
}

int unetdc_conv3x3_dgrad_colsum(const void* dy, int lddy, const void* w_dgrad, void* dx, int lddx, float* colsum, int c0,
                                int c, void* workspace, int64_t workspace_bytes, int n, int h, int w, int cin, int cout,
                                int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(dilation >= 1, "conv3x3_dgrad_colsum: dilation must be >= 1");
  UNETDC_REQUIRE(lddy >= cout && lddx >= cin, "conv3x3_dgrad_colsum: ld smaller than channel count");
  UNETDC_REQUIRE(colsum && workspace && c0 >= 0 && c > 0 && c0 + c <= cin, "conv3x3_dgrad_colsum: bad column range");
  if (workspace_bytes < unetdc_conv3x3_dgrad_colsum_workspace(n, h, w, cin)) {
    set_error("conv3x3_dgrad_colsum: workspace too small (%ld bytes)", (long)workspace_bytes);
    return UNETDC_EWORKSPACE;
  }
  IgemmParams p = conv3x3_igemm(n, h, w, cout, cin, lddy, lddx, dilation);
  p.x = dy; p.w = w_dgrad; p.out = dx; p.mode = MODE_STATS; p.stats = reinterpret_cast<float*>(workspace);
  int rc = launch_igemm(p, dtype, (hipStream_t)s);
  if (rc != UNETDC_OK) return rc;
  return launch_stats_colsum(p.stats, p.mblocks, cin, c0, c, colsum, (hipStream_t)s);       // rows the kernel wrote
}

// dgrad whose epilogue also produces the BatchNorm-backward partial sums of the stage that consumes dx
static int dgrad_bnstats_common(IgemmParams& p, const void* y_prev, int ldy_prev, const float* scale,
                                const float* shift, const float* mean, const float* rstd, float* parts,
                                int64_t parts_floats, int* nparts, int n, int h, int w, int c_prev, int dtype,
                                hipStream_t stream) {
  UNETDC_REQUIRE(y_prev && scale && shift && mean && rstd && parts && nparts, "dgrad_bnstats: null pointer");
  const int rows = igemm_mblocks((long)p.M, p.Cout);
  UNETDC_REQUIRE(partial_floats(rows, 3L * c_prev) <= parts_floats, "dgrad_bnstats: partial buffer too small");
  p.mode = MODE_BNBWD;
  p.stats = parts; p.bn_y = y_prev; p.bn_ldy = ldy_prev; p.scale = scale; p.shift = shift; p.bn_mean = mean; p.bn_rstd = rstd;
  if (plan_igemm(p, dtype).route != IGEMM_FIRSTGEN) {
    const int rc = launch_igemm(p, dtype, stream);
    if (rc == UNETDC_OK) *nparts = p.mblocks;                               // rows that carry data (<= rows; the rest are zeros)
    return rc;
  }
  // the first-generation kernel has no fused sums: plain dgrad, then the standalone reduction pass
  p.mode = MODE_STORE; p.stats = nullptr;
  const int rc = launch_igemm(p, dtype, stream);
  if (rc != UNETDC_OK) return rc;
  BnBwdParams b = bn_bwd_params(p.out, p.ldo, nullptr, 0, y_prev, ldy_prev, scale, shift, mean, rstd, nullptr, 0, n, h, w, c_prev);
  return launch_bn_bwd_reduce_only(b, parts, (long)parts_floats, nparts, dtype, stream);
}

int unetdc_conv3x3_dgrad_bnstats(const void* dy, int lddy, const void* w_dgrad, void* dx, int lddx,
                                            const void* y_prev, int ldy_prev, const float* scale, const float* shift,
                                            const float* mean, const float* rstd, float* parts, int64_t parts_floats,
                                            int* nparts, int n, int h, int w, int cin, int cout, int dilation,
                                            int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(dilation >= 1 && lddy >= cout && lddx >= cin, "conv3x3_dgrad_bnstats: bad dilation/ld");
  IgemmParams p = conv3x3_igemm(n, h, w, cout, cin, lddy, lddx, dilation);
  p.x = dy; p.w = w_dgrad; p.out = dx;
  return dgrad_bnstats_common(p, y_prev, ldy_prev, scale, shift, mean, rstd, parts, parts_floats, nparts, n, h, w,
                              cin, dtype, (hipStream_t)s);
}

int unetdc_convT2x2_dgrad_bnstats(const void* dup, int lddup, const void* w_dgrad, void* dx, int lddx,
                                             const void* y_prev, int ldy_prev, const float* scale, const float* shift,
                                             const float* mean, const float* rstd, float* parts,
                                             int64_t parts_floats, int* nparts, int n, int h, int w, int cin, int cout,
                                             int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(lddup >= cout && lddx >= cin, "convT2x2_dgrad_bnstats: ld smaller than channel count");
  IgemmParams p = convT2x2_dgrad_igemm(n, h, w, cin, cout, lddup, lddx);
  p.x = dup; p.w = w_dgrad; p.out = dx;
  return dgrad_bnstats_common(p, y_prev, ldy_prev, scale, shift, mean, rstd, parts, parts_floats, nparts, n, h, w,
                              cin, dtype, (hipStream_t)s);
}

int64_t unetdc_conv3x3_wgrad_workspace(int n, int h, int w, int cin, int cout, int dtype) {
  return wgrad_workspace_bound(n, h, w, cout, cin, 9, dtype);
}

int unetdc_conv3x3_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, void* workspace,
                         int64_t workspace_bytes, int n, int h, int w, int cin, int cout, int dilation, int dtype,
                         unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(dilation >= 1, "conv3x3_wgrad: dilation must be >= 1");
  WgradParams p = conv3x3_wgrad(n, h, w, cin, cout, ldx, lddy, dilation);
  p.a = dy; p.b = x;
  return launch_wgrad(p, dw, workspace, (long)workspace_bytes, dtype, (hipStream_t)s);
}

int unetdc_conv3x3_first_stats_rows(int64_t npixels, int cin, int cout) {
  return plan_first((long)npixels, cin, cout).fwd_blocks;
}

int unetdc_conv3x3_first_fwd(const float* x_nchw, const float* w, const float* bias, const float* scale,
                             const float* shift, void* y, int ldy, float* stats_part, int n, int h, int wd, int cin,
                             int cout, int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, wd);
  UNETDC_REQUIRE(dilation >= 1 && ldy >= cout, "conv3x3_first_fwd: bad dilation/ld");
  UNETDC_REQUIRE((scale == nullptr) == (shift == nullptr), "conv3x3_first_fwd: scale/shift mismatch");
  FirstParams p{};
  p.x = x_nchw; p.w = w; p.bias = bias; p.scale = scale; p.shift = shift; p.y = y; p.stats = stats_part;
  p.N = n; p.H = h; p.W = wd; p.Cin = cin; p.Cout = cout; p.ldy = ldy; p.dil = dilation;
  return launch_first_fwd(p, dtype, (hipStream_t)s);
}

int64_t unetdc_conv3x3_first_wgrad_workspace(int n, int h, int w, int cin, int cout) {
  return plan_first((long)n * h * w, cin, cout).workspace;
}

int unetdc_conv3x3_first_wgrad(const float* x_nchw, const void* dy, int lddy, float* dw, void* workspace,
                               int64_t workspace_bytes, int n, int h, int w, int cin, int cout, int dilation,
                               int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  FirstWgradParams p{};
  p.x = x_nchw; p.dy = dy; p.N = n; p.H = h; p.W = w; p.Cin = cin; p.Cout = cout; p.lddy = lddy; p.dil = dilation;
  return launch_first_wgrad(p, dw, workspace, (long)workspace_bytes, dtype, (hipStream_t)s);
}

int unetdc_conv3x3_first_wgrad_bn_supported(int n, int h, int w, int cin, int cout, int dilation, int dtype) {
  return first_wgrad_bn_supported(n, h, w, cin, cout, dilation, dtype) ? 1 : 0;
}

int unetdc_conv3x3_first_wgrad_bn(const float* x_nchw, const void* dz, int lddz, const void* y, int ldy, const float* scale,
                                  const float* shift, const float* mean, const float* rstd, const float* coeffs, float* dw,
                                  void* workspace, int64_t workspace_bytes, int n, int h, int w, int cin, int cout,
                                  int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(y != nullptr, "first_wgrad_bn: null saved output");
  FirstWgradParams p{};
  p.x = x_nchw; p.dy = dz; p.N = n; p.H = h; p.W = w; p.Cin = cin; p.Cout = cout; p.lddy = lddz; p.dil = dilation;
  p.bn_y = y; p.bn_ldy = ldy; p.bn_scale = scale; p.bn_shift = shift; p.bn_mean = mean; p.bn_rstd = rstd; p.bn_k = coeffs;
  return launch_first_wgrad(p, dw, workspace, (long)workspace_bytes, dtype, (hipStream_t)s);
}

int unetdc_bn_relu_bwd_coeffs(const float* pre_parts, int pre_nparts, const float* gamma, const float* rstd, float* dgamma,
                              float* dbeta, float* dbias, float* coeffs, int n, int h, int w, int c, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  return launch_bn_bwd_coeffs(pre_parts, pre_nparts, (long)n * h * w, gamma, rstd, dgamma, dbeta, dbias, coeffs, c, (hipStream_t)s);
}

int unetdc_conv3x3_first_dgrad(const void* dy, int lddy, const float* w, float* dx_nchw, int n, int h, int wd, int cin,
                               int cout, int dilation, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, wd);
  return launch_first_dgrad(dy, lddy, w, dx_nchw, n, h, wd, cin, cout, dilation, dtype, (hipStream_t)s);
}

int unetdc_convT2x2_fwd(const void* x, int ldx, const void* w_fwd, const float* bias, void* up, int ldup, int n,
                        int h, int w, int cin, int cout, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(ldx >= cin && ldup >= cout, "convT2x2_fwd: ld smaller than channel count");
  IgemmParams p{};
  p.x = x; p.w = w_fwd; p.out = up; p.bias = bias;
  p.M = n * h * w; p.Ho = h; p.Wo = w; p.Hi = h; p.Wi = w; p.Cin = cin; p.Cout = 4 * cout; p.ldx = ldx; p.ldo = ldup;
  p.ntaps = 1; p.stride = 1; p.mode = MODE_SHUFFLE; p.shuf_c = cout;
  p.offy[0] = 0; p.offx[0] = 0;
  return launch_igemm(p, dtype, (hipStream_t)s);
}

int unetdc_convT2x2_dgrad(const void* dup, int lddup, const void* w_dgrad, void* dx, int lddx, int n, int h, int w,
                          int cin, int cout, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  UNETDC_REQUIRE(lddup >= cout && lddx >= cin, "convT2x2_dgrad: ld smaller than channel count");
  IgemmParams p = convT2x2_dgrad_igemm(n, h, w, cin, cout, lddup, lddx);
  p.x = dup; p.w = w_dgrad; p.out = dx; p.mode = MODE_STORE;
  return launch_igemm(p, dtype, (hipStream_t)s);
}

int64_t unetdc_convT2x2_wgrad_workspace(int n, int h, int w, int cin, int cout, int dtype) {
  return wgrad_workspace_bound(n, h, w, cin, cout, 4, dtype);
}

int unetdc_convT2x2_wgrad(const void* x, int ldx, const void* dup, int lddup, float* dw, void* workspace,
                          int64_t workspace_bytes, int n, int h, int w, int cin, int cout, int dtype,
                          unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  WgradParams p{};
  p.a = x; p.b = dup; p.N = n; p.H = h; p.W = w; p.Hb = 2 * h; p.Wb = 2 * w; p.CI = cin; p.CJ = cout;
  p.lda = ldx; p.ldb = lddup; p.ntaps = 4; p.stride = 2;
  taps2x2(p.offy, p.offx);
  return launch_wgrad(p, dw, workspace, (long)workspace_bytes, dtype, (hipStream_t)s);
}

int unetdc_bn_finalize(const float* stats_part, int rows, int64_t count, const float* gamma, const float* beta,
                       float eps, float momentum, float* running_mean, float* running_var, float* scale,
                       float* shift, float* mean, float* rstd, int c, unetdc_stream_t s) {
  return launch_bn_finalize(stats_part, rows, (long)count, gamma, beta, eps, momentum, running_mean, running_var,
                            scale, shift, mean, rstd, c, (hipStream_t)s);
}

int unetdc_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, const float* conv_bias, float eps, float* scale, float* shift,
                          int c, unetdc_stream_t s) {
  return launch_bn_eval_affine(gamma, beta, running_mean, running_var, conv_bias, eps, scale, shift, c,
                               (hipStream_t)s);
}

int unetdc_bn_relu_apply(const void* y, int ldy, const float* scale, const float* shift, void* a, int lda,
                         void* pooled, int ldp, int n, int h, int w, int c, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  ApplyParams p{};
  p.y = y; p.a = a; p.pooled = pooled; p.scale = scale; p.shift = shift;
  p.N = n; p.H = h; p.W = w; p.C = c; p.ldy = ldy; p.lda = lda; p.ldp = ldp;
  return launch_apply(p, dtype, (hipStream_t)s);
}

int64_t unetdc_bn_relu_bwd_workspace(int n, int h, int w, int c, int pooled, int dtype) {
  return plan_bn_bwd(n, h, w, c, pooled, dtype).workspace;
}

int unetdc_bn_relu_bwd(const void* dskip, int ldskip, const void* dpool, int ldpool, const void* y, int ldy,
                       const float* scale, const float* shift, const float* mean, const float* rstd,
                       const float* gamma, void* dy, int lddy, float* dgamma, float* dbeta, float* dbias,
                       void* workspace, int64_t workspace_bytes, const float* pre_parts, int pre_nparts, int n, int h,
                       int w, int c, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  BnBwdParams p = bn_bwd_params(dskip, ldskip, dpool, ldpool, y, ldy, scale, shift, mean, rstd, dy, lddy, n, h, w, c);
  return launch_bn_bwd(p, gamma, dgamma, dbeta, dbias, workspace, (long)workspace_bytes, pre_parts, pre_nparts, dtype,
                       (hipStream_t)s, false);
}

int unetdc_bn_relu_bwd_head(const float* dprobs, const float* probs, const float* head_w, const void* y, int ldy,
                            const float* scale, const float* shift, const float* mean, const float* rstd,
                            const float* gamma, void* dy, int lddy, float* dgamma, float* dbeta, float* dbias,
                            void* workspace, int64_t workspace_bytes, const float* pre_parts, int pre_nparts, int n, int h,
                            int w, int c, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  BnBwdParams p = bn_bwd_params(nullptr, 0, nullptr, 0, y, ldy, scale, shift, mean, rstd, dy, lddy, n, h, w, c);
  p.head_dprobs = dprobs; p.head_probs = probs; p.head_w = head_w;
  UNETDC_REQUIRE(head_w != nullptr, "bn_relu_bwd_head: null head weights");
  return launch_bn_bwd(p, gamma, dgamma, dbeta, dbias, workspace, (long)workspace_bytes, pre_parts, pre_nparts, dtype,
                       (hipStream_t)s, false);
}

int unetdc_bn_frozen_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                            float eps, float* scale, float* shift, float* mean, float* rstd, int c, unetdc_stream_t s) {
  return launch_bn_frozen_affine(gamma, beta, running_mean, running_var, eps, scale, shift, mean, rstd, c, (hipStream_t)s);
}

int unetdc_bn_relu_bwd_frozen(const void* dskip, int ldskip, const void* dpool, int ldpool, const void* y, int ldy,
                              const float* scale, const float* shift, const float* mean, const float* rstd,
                              const float* gamma, void* dy, int lddy, float* dgamma, float* dbeta, float* dbias,
                              void* workspace, int64_t workspace_bytes, const float* pre_parts, int pre_nparts, int n, int h,
                              int w, int c, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, w);
  BnBwdParams p = bn_bwd_params(dskip, ldskip, dpool, ldpool, y, ldy, scale, shift, mean, rstd, dy, lddy, n, h, w, c);
  return launch_bn_bwd(p, gamma, dgamma, dbeta, dbias, workspace, (long)workspace_bytes, pre_parts, pre_nparts, dtype,
                       (hipStream_t)s, true);
}

int unetdc_head_fwd(const void* a, int lda, const float* w, const float* b, float* probs, int n, int h, int wd,
                    int c, int oc, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, wd);
  HeadParams p = head_params(a, lda, w, probs, nullptr, nullptr, 0, n, h, wd, c, oc);
  p.b = b;
  return launch_head_fwd(p, dtype, (hipStream_t)s);
}

int unetdc_head_fwd_bn(const void* y, int ldy, const float* scale, const float* shift, const float* w, const float* b,
                       float* probs, int n, int h, int wd, int c, int oc, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, wd);
  UNETDC_REQUIRE(y && scale && shift, "head_fwd_bn: null pointer");
  HeadParams p = head_params(y, ldy, w, probs, nullptr, nullptr, 0, n, h, wd, c, oc);
  p.b = b; p.bn_scale = scale; p.bn_shift = shift;
  return launch_head_fwd(p, dtype, (hipStream_t)s);
}

int64_t unetdc_head_bwd_workspace(int n, int h, int w, int c, int oc, int dtype) {
  return plan_head((long)n * h * w, c, oc, dtype, HEAD_BWD_MAX_ROWS).workspace;
}

int unetdc_head_bwd(const float* dprobs, const float* probs, const void* a, int lda, const float* w, void* da,
                    int ldda, float* dw, float* db, void* workspace, int64_t workspace_bytes, int n, int h, int wd,
                    int c, int oc, int dtype, unetdc_stream_t s) {
  GEOM_CHECK(n, h, wd);
  HeadParams p = head_params(a, lda, w, probs, dprobs, da, ldda, n, h, wd, c, oc);
  return launch_head_bwd(p, dw, db, workspace, (long)workspace_bytes, dtype, (hipStream_t)s, nullptr, 0);
}

int unetdc_head_bwd_bnstats(const float* dprobs, const float* probs, const void* a, int lda, const float* w, void* da,
                            int ldda, float* dw, float* db, void* workspace, int64_t workspace_bytes, const void* y_prev,
                            int ldy_prev, const float* scale, const float* shift, const float* mean, const float* rstd,
                            float* parts, int64_t parts_floats, int* nparts, int n, int h, int wd, int c, int oc, int dtype,
                            unetdc_stream_t s) {
  GEOM_CHECK(n, h, wd);
  UNETDC_REQUIRE(y_prev && scale && shift && mean && rstd && parts && nparts, "head_bwd_bnstats: null pointer");
  HeadParams p = head_params(a, lda, w, probs, dprobs, da, ldda, n, h, wd, c, oc);
  p.bn_y = y_prev; p.bn_ldy = ldy_prev; p.bn_scale = scale; p.bn_shift = shift; p.bn_mean = mean; p.bn_rstd = rstd;
  p.bn_parts = parts;
  return launch_head_bwd(p, dw, db, workspace, (long)workspace_bytes, dtype, (hipStream_t)s, nparts, (long)parts_floats);
}

int64_t unetdc_focal_dice_loss_workspace(int nimg, int64_t hw) { return loss_workspace_bytes(nimg, (long)hw); }

int unetdc_focal_dice_loss_fwd(const float* probs, const float* target, float* loss_out, float* coef, void* workspace,
                               int64_t workspace_bytes, int nimg, int64_t hw, float alpha, float gamma, float ratio,
                               float smooth, unetdc_stream_t s) {
  return launch_loss_fwd(probs, target, nullptr, loss_out, coef, workspace, (long)workspace_bytes, nimg, (long)hw, alpha, gamma,
                         ratio, smooth, (hipStream_t)s);
}

int unetdc_focal_dice_loss_bwd(const float* probs, const float* target, const float* coef, const float* grad_out,
                               float* dprobs, int nimg, int64_t hw, float alpha, float gamma, float ratio,
                               unetdc_stream_t s) {
  return launch_loss_bwd(probs, target, nullptr, coef, grad_out, dprobs, nimg, (long)hw, alpha, gamma, ratio, (hipStream_t)s);
}

int unetdc_focal_dice_loss_w_fwd(const float* probs, const float* target, const float* weight, float* loss_out, float* coef,
                                 void* workspace, int64_t workspace_bytes, int nimg, int64_t hw, float alpha, float gamma,
                                 float ratio, float smooth, unetdc_stream_t s) {
  UNETDC_REQUIRE(weight, "focal_dice_loss_w: null weight");
  return launch_loss_fwd(probs, target, weight, loss_out, coef, workspace, (long)workspace_bytes, nimg, (long)hw, alpha, gamma,
                         ratio, smooth, (hipStream_t)s);
}

int unetdc_focal_dice_loss_w_bwd(const float* probs, const float* target, const float* weight, const float* coef,
                                 const float* grad_out, float* dprobs, int nimg, int64_t hw, float alpha, float gamma,
                                 float ratio, unetdc_stream_t s) {
  UNETDC_REQUIRE(weight, "focal_dice_loss_w_bwd: null weight");
  return launch_loss_bwd(probs, target, weight, coef, grad_out, dprobs, nimg, (long)hw, alpha, gamma, ratio, (hipStream_t)s);
}

int64_t unetdc_border_weights_workspace(int n, int h, int w, int radius) { return border_workspace_bytes(n, h, w, radius); }

int unetdc_border_weights(const float* target, int n, int h, int w, float w0, float sigma, int radius, float* out_weight,
                          int32_t* out_d1, int32_t* out_d2, void* workspace, int64_t workspace_bytes, unetdc_stream_t s) {
  return launch_border_weights(target, n, h, w, w0, sigma, radius, out_weight, out_d1, out_d2, workspace, (long)workspace_bytes,
                               (hipStream_t)s);
}

// the bytes do not depend on the dtype, and a width that bf16 takes fp32 takes too
int64_t unetdc_channel_sum_workspace(int64_t npixels, int c) { return plan_channel_sum((long)npixels, c, UNETDC_F32).workspace; }

int unetdc_channel_sum(const void* x, int ldx, float* out, void* workspace, int64_t workspace_bytes,
                       int64_t npixels, int c, int dtype, unetdc_stream_t s) {
  return launch_channel_sum(x, ldx, out, workspace, (long)workspace_bytes, (long)npixels, c, dtype, (hipStream_t)s);
}

int unetdc_mask_from_probs(const float* probs, int ph, int pw, float thresh, uint8_t* mask, int oh, int ow,
                           unetdc_stream_t s) {
  return launch_mask_from_probs(probs, ph, pw, thresh, mask, oh, ow, (hipStream_t)s);
}

int unetdc_mask_from_probs_linear(const float* probs, int ph, int pw, float thresh, uint8_t* mask, int oh, int ow,
                                  const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                                  unetdc_stream_t s) {
  return launch_mask_from_probs_linear(probs, ph, pw, thresh, mask, oh, ow, xofs, xcoef, yofs, ycoef, (hipStream_t)s);
}

int64_t unetdc_ccl_workspace(int h, int w) { return ccl_workspace_bytes(h, w); }

int unetdc_ccl_stats(const uint8_t* mask, int h, int w, int min_area, void* workspace, int64_t workspace_bytes,
                     int32_t* out_count, int32_t* out_area, int64_t* out_sumy, int64_t* out_sumx, int32_t* out_root,
                     int max_out, unetdc_stream_t s) {
  return launch_ccl("ccl_stats", mask, h, w, min_area, workspace, (long)workspace_bytes, out_count, out_area,
                    reinterpret_cast<long long*>(out_sumy), reinterpret_cast<long long*>(out_sumx), out_root, nullptr, max_out,
                    (hipStream_t)s);
}

int64_t unetdc_split_workspace(int h, int w) { return split_workspace_bytes(h, w); }

int unetdc_edt_sq(const uint8_t* mask, int h, int w, int32_t* out_d2, void* workspace, int64_t workspace_bytes,
                  unetdc_stream_t s) {
  return launch_edt_sq(mask, h, w, out_d2, workspace, (long)workspace_bytes, (hipStream_t)s);
}

int unetdc_split_stats(const uint8_t* mask, int h, int w, int min_area, int split_depth_half_px, void* workspace,
                       int64_t workspace_bytes, int32_t* out_count, int32_t* out_area, int64_t* out_sumy, int64_t* out_sumx,
                       int32_t* out_root, int32_t* out_label, int max_out, unetdc_stream_t s) {
  return launch_split_stats(mask, h, w, min_area, split_depth_half_px, workspace, (long)workspace_bytes, out_count, out_area,
                            reinterpret_cast<long long*>(out_sumy), reinterpret_cast<long long*>(out_sumx), out_root,
                            out_label, max_out, (hipStream_t)s);
}

int64_t unetdc_ccl_labels_workspace(int h, int w) { return ccl_labels_workspace_bytes(h, w); }

int unetdc_ccl_labels(const uint8_t* mask, int h, int w, int min_area, void* workspace, int64_t workspace_bytes,
                      int32_t* out_count, int32_t* out_area, int64_t* out_sumy, int64_t* out_sumx, int32_t* out_root,
                      int32_t* out_label, int max_out, unetdc_stream_t s) {
  UNETDC_REQUIRE(out_label, "ccl_labels: null pointer");
  return launch_ccl("ccl_labels", mask, h, w, min_area, workspace, (long)workspace_bytes, out_count, out_area,
                    reinterpret_cast<long long*>(out_sumy), reinterpret_cast<long long*>(out_sumx), out_root, out_label,
                    max_out, (hipStream_t)s);
}

static_assert(UNETDC_SHAPE_QUANTITIES == SHAPE_QUANTITIES, "unetdc_label_props output rows");

int unetdc_label_props(const int32_t* label, const uint8_t* gray, int h, int w, int64_t* out, int max_out, unetdc_stream_t s) {
  return launch_label_props(label, gray, h, w, reinterpret_cast<long long*>(out), max_out, (hipStream_t)s);
}

static_assert(UNETDC_CONF_QUANTITIES == CONF_QUANTITIES && UNETDC_CONF_IMAGE_QUANTITIES == CONF_IMAGE_QUANTITIES,
              "unetdc_label_confidence output rows");

int unetdc_label_confidence(const int32_t* label, int max_out, int h, int w, const float* probs, const float* lo, const float* hi,
                            int ph, int pw, float thresh, float band, const uint16_t* entropy_table, int64_t* out,
                            int64_t* out_image, uint8_t* out_entropy_u8, uint8_t* out_spread_u8, unetdc_stream_t s) {
  return launch_label_confidence(label, max_out, h, w, probs, lo, hi, ph, pw, thresh, band, entropy_table,
                                 reinterpret_cast<long long*>(out), reinterpret_cast<long long*>(out_image), out_entropy_u8,
                                 out_spread_u8, (hipStream_t)s);
}

static_assert(UNETDC_HULL_QUANTITIES == HULL_QUANTITIES, "unetdc_label_hull output rows");

int64_t unetdc_label_hull_workspace(int h, int w, int max_out, int max_rows) { return label_hull_workspace_bytes(h, w, max_out, max_rows); }

int unetdc_label_hull(const int32_t* label, int max_out, int h, int w, void* workspace, int64_t workspace_bytes, int64_t* out,
                      int32_t* out_rows, int max_rows, unetdc_stream_t s) {
  return launch_label_hull(label, max_out, h, w, workspace, (long)workspace_bytes, reinterpret_cast<long long*>(out), out_rows,
                           max_rows, (hipStream_t)s);
}

static_assert(UNETDC_OUTLINE_QUANTITIES == OUTLINE_QUANTITIES && UNETDC_CONTOUR_FIELDS == CONTOUR_FIELDS, "unetdc_label_outlines output rows");

int64_t unetdc_label_outlines_workspace(int h, int w, int max_out, int max_cracks) { return label_outlines_workspace_bytes(h, w, max_out, max_cracks); }

int unetdc_label_outlines(const int32_t* label, int max_out, int h, int w, int max_len, void* workspace, int64_t workspace_bytes, int64_t* out,
                          int64_t* contours, int max_contours, int32_t* vx, int32_t* vy, int max_vertices, int max_cracks, int32_t* needed,
                          unetdc_stream_t s) {
  return launch_label_outlines(label, max_out, h, w, max_len, workspace, (long)workspace_bytes, reinterpret_cast<long long*>(out),
                               reinterpret_cast<long long*>(contours), max_contours, vx, vy, max_vertices, max_cracks, needed, (hipStream_t)s);
}

int64_t unetdc_polygon_fill_workspace(int h, int w, int n_polys, int n_rings, int n_verts) {
  return polygon_fill_workspace_bytes(h, w, n_polys, n_rings, n_verts);
}

int unetdc_polygon_fill(const int32_t* verts, const int32_t* ring_first, const int32_t* poly_first_ring, const int32_t* poly_label,
                        int n_polys, int n_rings, int n_verts, int h, int w, int32_t* labels_out, void* workspace,
                        int64_t workspace_bytes, unetdc_stream_t s) {
  return launch_polygon_fill(verts, ring_first, poly_first_ring, poly_label, n_polys, n_rings, n_verts, h, w, labels_out, workspace,
                             (long)workspace_bytes, (hipStream_t)s);
}

int unetdc_label_census(const int32_t* label, int h, int w, int n_labels, int64_t* area, unetdc_stream_t s) {
  return launch_label_census(label, h, w, n_labels, reinterpret_cast<long long*>(area), (hipStream_t)s);
}

int unetdc_label_relabel(int32_t* label, int h, int w, const int32_t* lut, int n_lut, unetdc_stream_t s) {
  return launch_label_relabel(label, h, w, lut, n_lut, (hipStream_t)s);
}

int64_t unetdc_label_overlap_workspace(int h, int w, int max_pairs) { return label_overlap_workspace_bytes(h, w, max_pairs); }

int unetdc_label_overlap(const int32_t* label_a, int max_a, const int32_t* label_b, int max_b, int h, int w, void* workspace,
                         int64_t workspace_bytes, int32_t* out_count, int32_t* out_a, int32_t* out_b, int32_t* out_n,
                         int max_pairs, unetdc_stream_t s) {
  return launch_label_overlap(label_a, max_a, label_b, max_b, h, w, workspace, (long)workspace_bytes, out_count, out_a, out_b,
                              out_n, max_pairs, (hipStream_t)s);
}

int64_t unetdc_label_neighbors_workspace(int h, int w, int max_label, int max_pairs) {
  return label_neighbors_workspace_bytes(h, w, max_label, max_pairs);
}

int unetdc_label_neighbors(const int32_t* label, int max_label, int h, int w, int radius, void* workspace,
                           int64_t workspace_bytes, int32_t* out_count, int32_t* out_a, int32_t* out_b, int32_t* out_d2,
                           int max_pairs, int32_t* out_nn_label, int32_t* out_nn_d2, int32_t* out_degree, int32_t* out_cluster,
                           int32_t* out_cluster_size, unetdc_stream_t s) {
  return launch_label_neighbors(label, max_label, h, w, radius, workspace, (long)workspace_bytes, out_count, out_a, out_b, out_d2,
                                max_pairs, out_nn_label, out_nn_d2, out_degree, out_cluster, out_cluster_size, (hipStream_t)s);
}

static_assert(UNETDC_CELL_DROPLET_QUANTITIES == CELL_DROPLET_QUANTITIES && UNETDC_CELL_QUANTITIES == CELL_QUANTITIES,
              "unetdc_cell_table output rows");

int64_t unetdc_label_nearest_workspace(int h, int w) { return label_nearest_workspace_bytes(h, w); }

int unetdc_label_nearest(const int32_t* label, int max_label, int h, int w, int radius, void* workspace, int64_t workspace_bytes,
                         int32_t* out_label, int32_t* out_d2, unetdc_stream_t s) {
  return launch_label_nearest(label, max_label, h, w, radius, workspace, (long)workspace_bytes, out_label, out_d2, (hipStream_t)s);
}

int64_t unetdc_cell_table_workspace(int h, int w, int max_droplet, int max_cell, int max_pairs) {
  return cell_table_workspace_bytes(h, w, max_droplet, max_cell, max_pairs);
}

int unetdc_cell_table(const int32_t* droplet_label, int max_droplet, const int32_t* cell_label, int max_cell, const int32_t* d2,
                      int h, int w, void* workspace, int64_t workspace_bytes, int32_t* out_needed, int max_pairs,
                      int32_t* out_droplet, int64_t* out_cell, unetdc_stream_t s) {
  return launch_cell_table(droplet_label, max_droplet, cell_label, max_cell, d2, h, w, workspace, (long)workspace_bytes, out_needed,
                           max_pairs, out_droplet, reinterpret_cast<long long*>(out_cell), (hipStream_t)s);
}

int64_t unetdc_ripley_workspace(int h, int w, int max_points, int rmax, int n_sim) {
  return ripley_workspace_bytes(h, w, max_points, rmax, n_sim);
}

int unetdc_droplet_points(const int32_t* count, const int32_t* area, const int64_t* sum_y, const int64_t* sum_x, int max_points,
                          const uint8_t* window, int h, int w, int32_t* out_py, int32_t* out_px, int32_t* out_info,
                          unetdc_stream_t s) {
  return launch_droplet_points(count, area, reinterpret_cast<const long long*>(sum_y), reinterpret_cast<const long long*>(sum_x),
                               max_points, window, h, w, out_py, out_px, out_info, (hipStream_t)s);
}

int unetdc_ripley_counts(const int32_t* py, const int32_t* px, const int32_t* n_points, int max_points, const uint8_t* window,
                         int h, int w, int rmax, int n_sim, uint32_t seed, void* workspace, int64_t workspace_bytes,
                         int32_t* out_n, int64_t* out_pairs, int64_t* out_pairs_all, unetdc_stream_t s) {
  return launch_ripley_counts(py, px, n_points, max_points, window, h, w, rmax, n_sim, seed, workspace, (long)workspace_bytes,
                              out_n, reinterpret_cast<long long*>(out_pairs), reinterpret_cast<long long*>(out_pairs_all),
                              (hipStream_t)s);
}

int64_t unetdc_boundary_distances_workspace(int h, int w) { return boundary_distances_workspace_bytes(h, w); }

int unetdc_boundary_distances(const int32_t* label_a, int max_a, const int32_t* label_b, int max_b, int h, int w, int radius,
                              void* workspace, int64_t workspace_bytes, int64_t* hist, int32_t* dmax, int64_t* out_a,
                              int64_t* out_b, unetdc_stream_t s) {
  return launch_boundary_distances(label_a, max_a, label_b, max_b, h, w, radius, workspace, (long)workspace_bytes,
                                   reinterpret_cast<long long*>(hist), dmax, reinterpret_cast<long long*>(out_a),
                                   reinterpret_cast<long long*>(out_b), (hipStream_t)s);
}

int64_t unetdc_mask_clean_workspace(int h, int w) { return mask_clean_workspace_bytes(h, w); }

int unetdc_mask_clean(const uint8_t* strong, const uint8_t* weak, int h, int w, int max_hole_area, void* workspace,
                      int64_t workspace_bytes, uint8_t* out_mask, int32_t* out_counts, unetdc_stream_t s) {
  return launch_mask_clean(strong, weak, h, w, max_hole_area, workspace, (long)workspace_bytes, out_mask, out_counts,
                           (hipStream_t)s);
}

int64_t unetdc_diff_regions_workspace(int h, int w) { return diff_regions_workspace_bytes(h, w); }

int unetdc_diff_regions(const uint8_t* pred, const uint8_t* gt, int h, int w, int min_area, void* workspace,
                        int64_t workspace_bytes, int64_t* out_image, int32_t* out_count, int32_t* out_class, int32_t* out_area,
                        int64_t* out_sumy, int64_t* out_sumx, int32_t* out_neighbors, int max_out, unetdc_stream_t s) {
  return launch_diff_regions(pred, gt, h, w, min_area, workspace, (long)workspace_bytes, reinterpret_cast<long long*>(out_image),
                             out_count, out_class, out_area, reinterpret_cast<long long*>(out_sumy),
                             reinterpret_cast<long long*>(out_sumx), out_neighbors, max_out, (hipStream_t)s);
}

int unetdc_diff_paint(const uint8_t* pred, const uint8_t* gt, const uint8_t* rgb, int h, int w, uint8_t* out_diff,
                      uint8_t* out_overlay, unetdc_stream_t s) {
  return launch_diff_paint(pred, gt, rgb, h, w, out_diff, out_overlay, (hipStream_t)s);
}

int unetdc_thresh_sweep(const float* probs, int n, int ph, int pw, const uint8_t* gt, int oh, int ow, const int32_t* xofs,
                        const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef, int k, int64_t* hist,
                        unetdc_stream_t s) {
  return launch_thresh_sweep(probs, n, ph, pw, gt, oh, ow, xofs, xcoef, yofs, ycoef, k, reinterpret_cast<long long*>(hist),
                             (hipStream_t)s);
}

int unetdc_tile_gather_u8_to_chw_f32(const uint8_t* src_hwc, int h, int w, int channels, float* tiles, int t, const int32_t* yo,
                                     int ny, const int32_t* xo, int nx, int t0, int count, unetdc_stream_t s) {
  return launch_tile_gather(src_hwc, h, w, channels, tiles, t, yo, ny, xo, nx, t0, count, (hipStream_t)s);
}

int unetdc_tile_blend_f32(const float* tile_probs, int t, int overlap, const int32_t* yo, int ny, const int32_t* xo, int nx,
                          float* out, int h, int w, unetdc_stream_t s) {
  return launch_tile_blend(tile_probs, t, overlap, yo, ny, xo, nx, out, h, w, (hipStream_t)s);
}

int unetdc_dihedral_expand_f32(const float* x, int n, int c, int s, int nvar, float* out, unetdc_stream_t stream) {
  return launch_dihedral_expand(x, n, c, s, nvar, out, (hipStream_t)stream);
}

int unetdc_dihedral_mean_f32(const float* p, int n, int s, int nvar, float* out, unetdc_stream_t stream) {
  return launch_dihedral_mean(p, n, s, nvar, out, (hipStream_t)stream);
}

int unetdc_dihedral_mean_env_f32(const float* p, int n, int s, int nvar, float* out_mean, float* out_lo, float* out_hi,
                                 unetdc_stream_t stream) {
  return launch_dihedral_mean_env(p, n, s, nvar, out_mean, out_lo, out_hi, (hipStream_t)stream);
}

int64_t unetdc_rolling_ball_workspace(int h, int w, int channels) { return rolling_ball_workspace_bytes(h, w, channels); }

int unetdc_rolling_ball_u8(const uint8_t* src_hwc, uint8_t* dst_hwc, int h, int w, int channels, int ksize, void* workspace,
                           int64_t workspace_bytes, unetdc_stream_t s) {
  return launch_rolling_ball(src_hwc, dst_hwc, h, w, channels, ksize, workspace, (long)workspace_bytes, (hipStream_t)s);
}

int unetdc_resize_linear_u8_to_chw_f32(const uint8_t* src_hwc, int h, int w, int channels, float* dst_chw, int dh, int dw,
                                       const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                                       unetdc_stream_t s) {
  return launch_resize_linear_chw(src_hwc, h, w, channels, dst_chw, dh, dw, xofs, xcoef, yofs, ycoef, (hipStream_t)s);
}

static_assert(sizeof(unetdc_augment_params) == sizeof(unetdc::AugRecord) &&
                  offsetof(unetdc_augment_params, beta_max) == offsetof(unetdc::AugRecord, beta_max),
              "unetdc_augment_params and AugRecord must share one layout");
static_assert(UNETDC_AUG_HFLIP == unetdc::AUG_HFLIP && UNETDC_AUG_VFLIP == unetdc::AUG_VFLIP && UNETDC_AUG_BC == unetdc::AUG_BC,
              "augmentation flag bits");

int64_t unetdc_elastic_fields_workspace(int n, int h, int w, double sigma) {
  return elastic_fields_workspace_bytes(n, h, w, sigma);
}

int unetdc_elastic_fields(const uint32_t* seeds, int n, int h, int w, double sigma, float alpha, float* fields,
                          void* workspace, int64_t workspace_bytes, unetdc_stream_t s) {
  return launch_elastic_fields(seeds, n, h, w, sigma, alpha, fields, workspace, (long)workspace_bytes, (hipStream_t)s);
}

int unetdc_augment_gather(const float* cache_img, const uint8_t* cache_mask, int ncache, int channels, int h, int w,
                          const unetdc_augment_params* params, int n, const float* fields, int nfields, float* out_img,
                          float* out_mask, unetdc_stream_t s) {
  return launch_augment_gather(cache_img, cache_mask, ncache, channels, h, w, reinterpret_cast<const AugRecord*>(params), n,
                               fields, nfields, out_img, out_mask, (hipStream_t)s);
}

// both public crop records are views of the one internal CropRecord: unetdc_crop_params names the last word `reserved`,
// unetdc_crop_scaled_params `t`
static_assert(sizeof(unetdc_crop_params) == 56 && sizeof(unetdc_crop_scaled_params) == 56 && sizeof(unetdc::CropRecord) == 56 &&
                  offsetof(unetdc_crop_params, mask_off) == offsetof(unetdc::CropRecord, mask_off) &&
                  offsetof(unetdc_crop_params, y0) == offsetof(unetdc::CropRecord, y0) &&
                  offsetof(unetdc_crop_params, field) == offsetof(unetdc::CropRecord, field) &&
                  offsetof(unetdc_crop_params, beta_max) == offsetof(unetdc::CropRecord, beta_max) &&
                  offsetof(unetdc_crop_params, reserved) == offsetof(unetdc::CropRecord, t) &&
                  offsetof(unetdc_crop_scaled_params, mask_off) == offsetof(unetdc::CropRecord, mask_off) &&
                  offsetof(unetdc_crop_scaled_params, y0) == offsetof(unetdc::CropRecord, y0) &&
                  offsetof(unetdc_crop_scaled_params, field) == offsetof(unetdc::CropRecord, field) &&
                  offsetof(unetdc_crop_scaled_params, beta_max) == offsetof(unetdc::CropRecord, beta_max) &&
                  offsetof(unetdc_crop_scaled_params, t) == offsetof(unetdc::CropRecord, t),
              "unetdc_crop_params, unetdc_crop_scaled_params and CropRecord must share one layout");

int unetdc_crop_gather(const uint8_t* images_u8, int64_t images_bytes, const uint8_t* masks_u8, int64_t masks_bytes, int channels,
                       int S, const unetdc_crop_params* records, int n, const float* fields, int nfields, float* out_img,
                       float* out_mask, unetdc_stream_t s) {
  return launch_crop_gather("crop_gather", false, images_u8, (long)images_bytes, masks_u8, (long)masks_bytes, channels, S,
                            reinterpret_cast<const CropRecord*>(records), n, fields, nfields, out_img, out_mask, (hipStream_t)s);
}

int unetdc_crop_gather_scaled(const uint8_t* images_u8, int64_t images_bytes, const uint8_t* masks_u8, int64_t masks_bytes,
                              int channels, int S, const unetdc_crop_scaled_params* records, int n, const float* fields,
                              int nfields, float* out_img, float* out_mask, unetdc_stream_t s) {
  return launch_crop_gather("crop_gather_scaled", true, images_u8, (long)images_bytes, masks_u8, (long)masks_bytes, channels, S,
                            reinterpret_cast<const CropRecord*>(records), n, fields, nfields, out_img, out_mask, (hipStream_t)s);
}

int64_t unetdc_density_workspace(int h, int w) { return density_workspace_bytes(h, w); }

static_assert(sizeof(unetdc_density_stats) == 1088 && offsetof(unetdc_density_stats, max_ring_distance) == 40 &&
                  offsetof(unetdc_density_stats, ring_count) == 68,
              "unetdc_density_stats layout (unet_dc_segmentation_amd/density.py:STATS_DTYPE mirrors it)");

int unetdc_density_maps(const uint8_t* rgb_hwc, const uint8_t* mask, int h, int w, const int32_t* droplet_count,
                        const int32_t* droplet_area, const int64_t* droplet_sumy, const int64_t* droplet_sumx,
                        int max_droplets, int nb_layers, double sigma, const double* taps, void* workspace,
                        int64_t workspace_bytes, unetdc_density_stats* out_stats, uint8_t* out_radial_index,
                        uint8_t* out_spatial_index, uint8_t* out_blur, uint8_t* out_roi, uint8_t* out_ring,
                        float* out_radial, float* out_spatial, unetdc_stream_t s) {
  return launch_density_maps(rgb_hwc, mask, h, w, droplet_count, droplet_area,
                             reinterpret_cast<const long long*>(droplet_sumy), reinterpret_cast<const long long*>(droplet_sumx),
                             max_droplets, nb_layers, sigma, taps, workspace, (long)workspace_bytes, out_stats,
                             out_radial_index, out_spatial_index, out_blur, out_roi, out_ring, out_radial, out_spatial,
                             (hipStream_t)s);
}

int unetdc_density_sqrt(const int64_t* x, double* out, int64_t n, unetdc_stream_t s) {
  return launch_density_sqrt(reinterpret_cast<const long long*>(x), out, (long)n, (hipStream_t)s);
}

int64_t unetdc_u16_ranks_workspace(int h, int w, int c, int nq) { return u16_ranks_workspace_bytes(h, w, c, nq); }

int unetdc_u16_ranks(const uint16_t* src, int h, int w, int c, const int32_t* ppm, int nq, void* workspace, int64_t workspace_bytes,
                     int32_t* out_value, int32_t* out_below, int32_t* out_equal, unetdc_stream_t s) {
  return launch_u16_ranks(src, h, w, c, ppm, nq, workspace, (long)workspace_bytes, out_value, out_below, out_equal, (hipStream_t)s);
}

int unetdc_window_u16_to_u8(const uint16_t* src, int h, int w, int c, const int32_t* levels, uint8_t* dst, int dc,
                            unetdc_stream_t s) {
  return launch_window_u16_to_u8(src, h, w, c, levels, dst, dc, (hipStream_t)s);
}

int unetdc_planes_max_u16(const uint16_t* src, int planes, int h, int w, uint16_t* dst, unetdc_stream_t s) {
  return launch_planes_max_u16(src, planes, h, w, dst, (hipStream_t)s);
}

}  // extern "C"
