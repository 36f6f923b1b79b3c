// Parameter blocks and host launchers shared between the kernel files and the C-ABI layer.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "workspace.h"
#include "../../include/unetdc_hip.h"

namespace unetdc {

// MODE_BNBWD: plain store of a gradient tensor dA plus, fused, the per-channel partial sums of the
// BatchNorm-backward reduction of the stage that consumes dA:  S1 = sum dA*[n>0], S2 = sum dA*[n>0]*xhat
// with n = scale*y + shift, xhat = (y - mean)*rstd read from that stage's saved conv output y.
enum { MODE_STORE = 0, MODE_STATS = 1, MODE_AFFINE_RELU = 2, MODE_SHUFFLE = 3, MODE_BNBWD = 4 };
#define UNETDC_EUNSUPPORTED (-4)

struct IgemmParams {
  const void* x;
  const void* w;
  void* out;
  const float* bias;
  const float* scale;
  const float* shift;
  float* stats;
  const void* bn_y;          // MODE_BNBWD: saved conv output of the consuming stage, [M][bn_ldy]
  const float* bn_mean;
  const float* bn_rstd;
  int bn_ldy;
  int M, Ho, Wo, Hi, Wi, Cin, Cout, ldx, ldo, ntaps, stride, mode, shuf_c;
  int mblocks, nblocks;
  int wo_shift, howo_shift;  // log2(Wo), log2(Ho*Wo) when both are powers of two, else -1 (set by launch_igemm)
  int quad_bpr, quad_bpi;    // > 0: the M index walks 16 x 16 pixel blocks (blocks per image row / per image), see igemm_dma16.hip
  // input normalisation ("bnin"): x is the RAW conv output of the producing stage; its BatchNorm + ReLU, relu(in_scale * x +
  // in_shift) rounded through the storage type, is applied to every staged patch in LDS (igemm_lattice.hip, INORM)
  const float* in_scale;
  const float* in_shift;
  // optional (wide INORM form): the normalised activation is ALSO written out, [M][ld_act], by the items of n-block 0 -- the
  // weight gradient of the stage then reads a stored activation (plain kernel) without a stand-alone normalisation pass
  void* act_out;
  int ld_act;
  int offy[9];
  int offx[9];
};
// The kernel family of an implicit-GEMM call, decided once by plan_igemm (igemm_conv.hip).
enum IgemmRoute {
  IGEMM_UNSUPPORTED = 0,  // input normalisation asked for a shape the lattice kernel does not take
  IGEMM_LATTICE,          // igemm_lattice.hip: persistent lattice-halo conv (bf16), the only one with input normalisation
  IGEMM_HALO,             // igemm_halo.hip: LDS-staged input patch shared by all 9 taps (narrow layers, d <= 2)
  IGEMM_DMA,              // igemm_dma.hip: second generation, tensors < 2 GiB
  IGEMM_DMA16,            // igemm_dma16.hip: the same on the 16x16x32 bf16 MFMA shape
  IGEMM_FIRSTGEN,         // igemm_conv.hip: any size; no fused BatchNorm-backward sums
};
struct IgemmPlan {
  int route;
  int cfg;          // DMA / DMA16 tile: 1 = 256x256, 2 = 256x128, 3 = 256x64; first generation: 1 = 128x128, 0 = 256x64
  bool writes_act;  // input normalisation: the form can also store the normalised activation (IgemmParams::act_out)
};
IgemmPlan plan_igemm(const IgemmParams& p, int dtype);
int launch_igemm(IgemmParams& p, int dtype, hipStream_t stream);
int igemm_mblocks(long M, int Cout);
bool igemm_lattice_supported(const IgemmParams& p, int dtype);
bool igemm_halo_supported(const IgemmParams& p, int dtype);
int launch_igemm_lattice(IgemmParams& p, hipStream_t stream);
int launch_igemm_halo(IgemmParams& p, int dtype, hipStream_t stream);
int launch_igemm_dma(IgemmParams& p, int cfg, int dtype, hipStream_t stream);
int launch_igemm_dma16(IgemmParams& p, int cfg, hipStream_t stream);

struct WgradParams {
  const void* a;
  const void* b;
  float* part;
  int N, H, W, Hb, Wb, CI, CJ, lda, ldb, ntaps, stride;
  int P;            // N*H*W
  int chunk;        // pixels per K-slice (multiple of the block's pixel step)
  int ksplit, itiles, jtiles;
  int adv_y, adv_x; // pixel step decomposed: step = adv_y*W + adv_x
  int offy[9];
  int offx[9];
  const float* in_scale;   // "bnin": b (the conv input) is the RAW output of the producing stage, normalised on load
  const float* in_shift;
};
// The kernel of a weight gradient and its sizing, decided once by plan_wgrad (wgrad.hip).
enum WgradRoute {
  WGRAD_UNSUPPORTED = 0,  // input normalisation asked for a shape the tap-split ring kernel does not take
  WGRAD_CONVT,            // convt_wgrad.hip: tap-fused ConvTranspose2d(2, 2) (bf16), X staged once for the four taps
  WGRAD_RECT,             // wgrad_rect.hip: valid-rectangle kernel for strongly dilated 3x3 layers (bf16)
  WGRAD_FUSED,            // wgrad_fused.hip: tap-fused ring / tap-split kernels for narrow 3x3 layers
  WGRAD_DMA,              // wgrad_dma.hip: K split over the pixels, second generation (operands < 2 GiB)
  WGRAD_LEGACY,           // wgrad.hip: K split over the pixels, first generation
};
// Kernel variant and sizing of the tap-fused route, decided once by plan_wgrad_fused (wgrad_fused.hip): a pure host function.
struct WgradFusedPlan {
  bool supported;       // the route takes the call (with WgradParams::in_scale set: its input-normalising form does)
  bool paired;          // 512-thread workgroups: two halves walk the two halves of a unit's rows and meet in LDS
  bool bnin;            // X rows are normalised in LDS
  int pf;               // prefetch stages of the ring kernels (1 | 2); 0: three-segment staging
  int ysplit, rows_per_unit, imgs_per_unit, half_lds;   // -> WgradFusedParams
  int threads, nwg;     // workgroup size and count
  int lds, lds_attr;    // dynamic LDS bytes of the launch; the kernel's dynamic-LDS attribute
  int units;            // slabs to reduce
  long workspace;       // slab bytes asked of the caller: wgrad_fused_workspace_bytes, >= units * 9 * CI * CJ * 4
};
struct WgradPlan {
  int route;
  WgradFusedPlan fused; // WGRAD_FUSED
  int ksplit;           // K split (DMA / legacy / ConvT): slabs to reduce; rect: K units of all taps
  int chunk, tw, step;  // DMA / legacy: pixels per K slice, tile width in 64-channel units, pixel step of a block
  int steps_per_half;   // ConvT
  long workspace;       // bytes of partial slabs the route needs
};
WgradPlan plan_wgrad(const WgradParams& p, int dtype);
long wgrad_workspace_bound(int N, int H, int W, int CI, int CJ, int ntaps, int dtype);
int launch_wgrad(WgradParams& p, float* out, void* workspace, long workspace_bytes, int dtype, hipStream_t stream);
bool convt_wgrad_split(int N, int H, int W, int CI, int CJ, int& ksplit, int& steps_per_half);
int launch_convt_wgrad_fused(const WgradParams& w, const WgradPlan& pl, hipStream_t stream);
int wgrad_rect_units(int N, int H, int W, int CI, int CJ, int d);
int launch_wgrad_rect(const WgradParams& w, const WgradPlan& pl, float* out, hipStream_t stream);
WgradFusedPlan plan_wgrad_fused(const WgradParams& w, int dtype);
long wgrad_fused_workspace_bytes(int N, int H, int W, int CI, int CJ, int dtype);
int launch_wgrad_fused(const WgradParams& w, const WgradFusedPlan& pl, int dtype, hipStream_t stream);
int wgrad_dma_tile(int CI, int CJ);
int wgrad_dma_pixel_step(int dtype, int tw);
int launch_wgrad_dma_kernel(WgradParams& p, int tw, int dtype, hipStream_t stream);

struct FirstParams {
  const float* x;        // [N][Cin][H][W] fp32
  const float* w;        // [Cout][Cin][3][3] fp32 (PyTorch layout)
  const float* bias;     // [Cout] or null
  const float* scale;    // eval mode: y = relu(acc*scale + shift)
  const float* shift;
  void* y;               // [N*H*W][ldy] T
  float* stats;          // [gridDim.x][2][Cout] or null
  int N, H, W, Cin, Cout, ldy, dil;
};
struct FirstWgradParams {
  const float* x;     // [N][Cin][H][W]
  const void* dy;     // [P][lddy] T
  float* part;        // [gridDim.x][Cin][9][Cout]
  int N, H, W, Cin, Cout, lddy, dil;
  // "bn" form (row-run kernel, Cin = 1): `dy` is the gradient of the stage's ACTIVATED output and the BatchNorm + ReLU backward
  // of the stage is applied on load, dy = k1 * [a > 0] * dz - k2 - k3 * xhat rounded through the storage type (exactly what the
  // stand-alone pass would have stored) from the saved conv output y and the coefficients of unetdc_bn_relu_bwd_coeffs
  const void* bn_y; int bn_ldy;
  const float* bn_scale; const float* bn_shift; const float* bn_mean; const float* bn_rstd; const float* bn_k;   // bn_k: [3][Cout]
};
// The first layer's kernels and grids, decided once by plan_first (first_conv.hip).
struct FirstPlan {
  bool mfma;          // forward on the matrix cores (first_conv_mfma.hip), else the VALU kernel
  int fwd_blocks;     // forward grid = rows of partial statistics
  bool wgrad_mfma;    // weight gradient on the matrix cores, else a VALU kernel
  int wgrad_blocks;   // grid of the MFMA / general VALU weight-gradient kernel
  int rows_blocks;    // grid of the VALU row-run kernel (0 with the MFMA kernel)
  long workspace;     // bytes of partial slabs that cover the weight-gradient kernel a launch can pick
};
FirstPlan plan_first(long P, int Cin, int Cout);
int launch_first_fwd(FirstParams& p, int dtype, hipStream_t stream);
bool first_wgrad_bn_supported(int N, int H, int W, int Cin, int Cout, int dil, int dtype);
int launch_bn_bwd_coeffs(const float* pre_parts, int pre_nparts, long count, const float* gamma, const float* rstd, float* dgamma,
                         float* dbeta, float* dbias, float* coeffs, int C, hipStream_t stream);
int first_mfma_mblocks(long P);
int first_mfma_wgrad_blocks(long P);
int launch_first_mfma_fwd(FirstParams& p, int blocks, int dtype, hipStream_t stream);
int launch_first_mfma_wgrad(FirstWgradParams& p, int blocks, int dtype, hipStream_t stream);
int launch_first_wgrad(FirstWgradParams& p, float* dw, void* workspace, long workspace_bytes, int dtype,
                       hipStream_t stream);
int launch_first_dgrad(const void* dy, int lddy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, int dil,
                       int dtype, hipStream_t stream);

struct ApplyParams {
  const void* y; void* a; void* pooled;
  const float* scale; const float* shift;
  int N, H, W, C, ldy, lda, ldp;
};
struct BnBwdParams {
  const void* dskip; const void* dpool; const void* y; void* dy;
  const float* scale; const float* shift; const float* mean; const float* rstd;
  const float* k1; const float* k2; const float* k3;
  float* parts;            // [gridDim.x][3][C]
  int N, H, W, C, lds, ldp, ldy, lddy;
  // the stage feeds the 1 x 1 head with ONE output channel: its activation gradient is dz * w[c], dz = dprobs * p * (1 - p)
  // per pixel -- recomputed here from the fp32 [N, 1, H, W] tensors instead of being stored by the head backward and read
  // back (non-pooled apply pass only; rounded through the storage type like the stored tensor was)
  const float* head_dprobs; const float* head_probs; const float* head_w;
};
struct HeadParams {
  const void* a; const float* w; const float* b; float* probs;
  const float* dprobs; void* da; float* parts;      // backward
  int N, H, W, C, OC, lda, ldda;
  // optional: BatchNorm-backward partial sums of the stage that produced `a` (its saved conv output y + batch statistics)
  const void* bn_y; const float* bn_scale; const float* bn_shift; const float* bn_mean; const float* bn_rstd;
  float* bn_parts;  // [gridDim.x][3][C]
  int bn_ldy;
};
// ---- the HBM-bound operators: partials.hip, batchnorm.hip, head.hip, pack.hip ----
// Spare-row contract of the two-stage reductions (reduce_parts, partials.hip): a buffer of `rows` partial rows of L floats
// carries SPARE_ROWS more rows behind them, where the first stage leaves its <= SPARE_ROWS reduced rows.
constexpr int SPARE_ROWS = 64;
inline long partial_floats(long rows, long L) { return (rows + SPARE_ROWS) * L; }    // floats of such a buffer
inline long partial_row_cap(long floats, long L) { return floats / L - SPARE_ROWS; } // rows a caller-sized buffer takes
inline int chunk_elems(int dtype) { return dtype == UNETDC_BF16 ? 8 : dtype == UNETDC_F32 ? 4 : 0; }   // 0: no such dtype
inline int grid_for(long work_items, int per_block, long cap = 8192) {
  return (int)std::min(std::max((work_items + per_block - 1) / per_block, 1L), cap);
}
// One launch line per kernel: f(TypeTag<T>{}, std::bool_constant...) for the dtype (valid: chunk_elems) and run-time flags.
template <typename T> struct TypeTag { using type = T; };
template <typename F> void dispatch_flags(F&& f) { f(); }
template <typename F, typename... B> void dispatch_flags(F&& f, bool b, B... rest) {
  if (b) dispatch_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else dispatch_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <typename F, typename... B> void dispatch(int dtype, F&& f, B... flags) {
  if (dtype == UNETDC_BF16) dispatch_flags([&](auto... c) { f(TypeTag<bf16_t>{}, c...); }, flags...);
  else dispatch_flags([&](auto... c) { f(TypeTag<float>{}, c...); }, flags...);
}
// Host-only plans, decided once: the *_workspace query, the launcher and the reduce-only pass all read them.  ok == false
// (and workspace == 0): a dtype or width the launcher refuses.  epc, cpp: elements per chunk, chunks per pixel.
// seg: chunk lanes of a workgroup row; reduce grid (nb, ny) = partial rows x chunk segments; apply grid (apply_nb, ny);
// workspace bytes: [3][C] coefficients + partial_floats(nb, 3 C)
struct BnBwdPlan { bool ok; int epc, cpp, seg, nb, ny, apply_nb; long workspace; };
BnBwdPlan plan_bn_bwd(int N, int H, int W, int C, int pooled, int dtype);
// cpp = lanes per pixel: a power of two <= 64; bwd_nb = partial rows <= row_cap; workspace (backward): partial_floats(bwd_nb, OC (C + 1))
struct HeadPlan { bool ok; int epc, cpp, fwd_nb, bwd_nb; long workspace; };
constexpr long HEAD_BWD_MAX_ROWS = 1024;
HeadPlan plan_head(long P, int C, int OC, int dtype, long row_cap);
struct ChannelSumPlan { bool ok; int epc, nb, ny; long workspace; };   // workspace bytes: partial_floats(nb, C)
ChannelSumPlan plan_channel_sum(long P, int C, int dtype);

int launch_bn_finalize(const float* parts, int nparts, long count, const float* gamma, const float* beta, float eps,
                       float momentum, float* rm, float* rv, float* scale, float* shift, float* mean, float* rstd,
                       int C, hipStream_t stream);
int launch_bn_eval_affine(const float* gamma, const float* beta, const float* rm, const float* rv,
                          const float* conv_bias, float eps, float* scale, float* shift, int C, hipStream_t stream);
int launch_apply(ApplyParams& p, int dtype, hipStream_t stream);
int launch_bn_bwd(BnBwdParams& p, const float* gamma, float* dgamma, float* dbeta, float* dbias, void* workspace,
                  long workspace_bytes, const float* pre_parts, int pre_nparts, int dtype, hipStream_t stream, bool frozen);
int launch_bn_frozen_affine(const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* scale,
                            float* shift, float* mean, float* rstd, int C, hipStream_t stream);
int launch_bn_bwd_reduce_only(BnBwdParams& p, float* parts, long parts_floats, int* nparts, int dtype, hipStream_t stream);
int launch_head_fwd(HeadParams& p, int dtype, hipStream_t stream);
// bn_nparts / bn_parts_floats: the fused BatchNorm-backward sums (HeadParams::bn_y set), else null / 0
int launch_head_bwd(HeadParams& p, float* dw, float* db, void* workspace, long workspace_bytes, int dtype,
                    hipStream_t stream, int* bn_nparts, long bn_parts_floats);
int launch_pack_conv3x3(const float* w, void* wf, void* wd, int Co, int Ci, int dtype, hipStream_t stream);
int launch_pack_convT2x2(const float* w, void* wf, void* wd, int Ci, int Co, int dtype, hipStream_t stream);
int launch_pack_many(const void* table_dev, int n, long total, int dtype, hipStream_t stream);
int launch_adam_step(const void* table_dev, int n, long total_blocks, const float* flat_grad, double lr, double beta1,
                     double beta2, double eps, long step, double grad_scale, int dtype, hipStream_t stream);   // optim.hip
// the optimizer recipe: global gradient norm -> unetdc_step_ctl, and the step that reads it
long grad_norm_workspace_bytes(long n);                     // 0 for n <= 0
int launch_grad_norm(const float* flat_grad, long n, double grad_scale, double max_norm, void* ctl_dev, void* workspace,
                     long workspace_bytes, hipStream_t stream);
int launch_adam_step_ex(const void* table_dev, int n, long total_blocks, const float* flat_grad, double lr, double beta1,
                        double beta2, double eps, long step, double grad_scale, int dtype, const void* ctl_dev,
                        double weight_decay, float* ema_base, const float* m_base, double ema_decay, hipStream_t stream);
int launch_stats_colsum(const float* parts, int nparts, int ctotal, int c0, int c, float* out, hipStream_t stream);
int launch_channel_sum(const void* x, int ldx, float* out, void* workspace, long workspace_bytes, long P, int C,
                       int dtype, hipStream_t stream);

// ccl.hip: droplet quantification
int launch_mask_from_probs(const float* probs, int ph, int pw, float thresh, unsigned char* mask, int oh, int ow,
                           hipStream_t stream);
int launch_mask_from_probs_linear(const float* probs, int ph, int pw, float thresh, unsigned char* mask, int oh, int ow,
                                  const int* xofs, const short* xcoef, const int* yofs, const short* ycoef, hipStream_t stream);
// out_label null: unetdc_ccl_stats, else unetdc_ccl_labels (the larger workspace); who: the entry point's name for the messages
long ccl_workspace_bytes(int h, int w);
long ccl_labels_workspace_bytes(int h, int w);
int launch_ccl(const char* who, const unsigned char* mask, int h, int w, int min_area, void* workspace, long workspace_bytes,
               int* out_count, int* out_area, long long* out_sumy, long long* out_sumx, int* out_root, int* out_label,
               int max_out, hipStream_t stream);
// the stages of launch_ccl around its merge kernel, for split.hip: the layout of a ccl workspace with `extra` more int32
// planes of h * w words behind it (more), their initialisation (L[i] = i, sums 0), and per-class sums -> min_area
// filter -> raster-order compaction on whatever union-find the caller left in L.  rank_of_root (nullable, [h * w]) receives the
// 1-based output rank at the root pixel of every kept class.  No checks, no check_launch: the caller does both.
struct CclPlanes {
  unsigned long long *sy, *sx;
  int *L, *area, *blocksum;
};
struct CclWorkspace {
  CclPlanes ccl;
  int* more;
};
Layout<CclWorkspace> ccl_layout(int h, int w, int extra, void* workspace);
void launch_ccl_init(const unsigned char* mask, const CclPlanes& p, int n, hipStream_t stream);
void launch_ccl_finish(const unsigned char* mask, int h, int w, int min_area, const CclPlanes& p, int* out_count,
                       int* out_area, long long* out_sumy, long long* out_sumx, int* out_root, int* rank_of_root, int max_out,
                       hipStream_t stream);
// label[i] = rank_of_root[L[i]] on the foreground pixels of classes with at least min_area pixels, 0 elsewhere (after
// launch_ccl_finish, which compresses L and fills rank_of_root)
void launch_ccl_label(const unsigned char* mask, const CclPlanes& p, const int* rank_of_root, int min_area, int* label, int n,
                      hipStream_t stream);
// the scan of launch_ccl_finish alone, for diffmap.hip: blocksum[0 .. nblocks) (nblocks <= 2^20) -> its exclusive prefix sums
// in place, *total = the sum
void launch_ccl_scan(int* blocksum, int nblocks, int* total, hipStream_t stream);

// shape.hip: per-label second moments, bounding box, perimeter classes and grey statistics of an int32 label map
constexpr int SHAPE_QUANTITIES = 14;
int launch_label_props(const int* label, const unsigned char* gray, int h, int w, long long* out, int max_out,
                       hipStream_t stream);

// confidence.hip: per-label and per-image integers of the quantised probability, its entropy and the TTA envelope under an
// int32 label map
constexpr int CONF_QUANTITIES = 10, CONF_IMAGE_QUANTITIES = 8;
int launch_label_confidence(const int* label, int max_out, int h, int w, const float* probs, const float* lo, const float* hi,
                            int ph, int pw, float thresh, float band, const unsigned short* table, long long* out,
                            long long* out_image, unsigned char* out_entropy, unsigned char* out_spread, hipStream_t stream);

// match.hip: the sparse contingency table of two int32 label maps, in (a, b) order
long label_overlap_workspace_bytes(int h, int w, int max_pairs);
int launch_label_overlap(const int* label_a, int max_a, const int* label_b, int max_b, int h, int w, void* workspace,
                         long workspace_bytes, int* out_count, int* out_a, int* out_b, int* out_n, int max_pairs,
                         hipStream_t stream);

// hull.hip: twice the hull area, the largest squared vertex distance, the minimum-width edge's (Wc, Wl) and the vertex count of
// the convex hull of the pixel squares of every label of an int32 label map
constexpr int HULL_QUANTITIES = 5;
long label_hull_workspace_bytes(int h, int w, int max_out, int max_rows);               // 0 for arguments the call refuses
int launch_label_hull(const int* label, int max_out, int h, int w, void* workspace, long workspace_bytes, long long* out,
                      int* out_rows, int max_rows, hipStream_t stream);

// outlines.hip: the ordered contours (crack following as list ranking) of every label of an int32 label map, six integers per
// label, the contour table and the vertex lists
constexpr int OUTLINE_QUANTITIES = 6;
constexpr int CONTOUR_FIELDS = 5;
long label_outlines_workspace_bytes(int h, int w, int max_out, int max_cracks);        // 0 for arguments the call refuses
int launch_label_outlines(const int* label, int max_out, int h, int w, int max_len, void* workspace, long workspace_bytes, long long* out,
                          long long* contours, int max_contours, int* vx, int* vy, int max_vertices, int max_cracks, int* needed,
                          hipStream_t stream);

// polyfill.hip: polygons -> int32 label map by the exact even-odd rule at pixel centres, the census of a label map's values and
// a lookup applied in place
long polygon_fill_workspace_bytes(int h, int w, int n_polys, int n_rings, int n_verts);       // -1 for arguments the call refuses
int launch_polygon_fill(const int* verts, const int* ring_first, const int* poly_first_ring, const int* poly_label, int n_polys,
                        int n_rings, int n_verts, int h, int w, int* labels_out, void* workspace, long workspace_bytes,
                        hipStream_t stream);
int launch_label_census(const int* label, int h, int w, int n_labels, long long* area, hipStream_t stream);
int launch_label_relabel(int* label, int h, int w, const int* lut, int n_lut, hipStream_t stream);

// neighbors.hip: contact pairs, nearest contact, degree and cluster of the labels of an int32 label map
long label_neighbors_workspace_bytes(int h, int w, int max_label, int max_pairs);       // 0 for arguments the call refuses
int launch_label_neighbors(const int* label, int max_label, int h, int w, int radius, void* workspace, long workspace_bytes,
                           int* out_count, int* out_a, int* out_b, int* out_d2, int max_pairs, int* out_nn_label,
                           int* out_nn_d2, int* out_degree, int* out_cluster, int* out_cluster_size, hipStream_t stream);

// cells.hip: the nearest-label transform of a seed label map and the per-cell reduction of the droplet table (DESIGN.md
// section 31; include/unetdc_hip.h)
constexpr int CELL_DROPLET_QUANTITIES = 6;
constexpr int CELL_QUANTITIES = 8;
long label_nearest_workspace_bytes(int h, int w);                                       // 0 for arguments the call refuses
int launch_label_nearest(const int* label, int max_label, int h, int w, int radius, void* workspace, long workspace_bytes,
                         int* out_label, int* out_d2, hipStream_t stream);
long cell_table_workspace_bytes(int h, int w, int max_droplet, int max_cell, int max_pairs);   // 0 likewise
int launch_cell_table(const int* droplet_label, int max_droplet, const int* cell_label, int max_cell, const int* d2, int h, int w,
                      void* workspace, long workspace_bytes, int* out_needed, int max_pairs, int* out_droplet, long long* out_cell,
                      hipStream_t stream);

// spatial.hip: centroid pixels of a droplet table; Ripley counts of the observed pattern and of simulated ones (DESIGN.md
// section 26)
long ripley_workspace_bytes(int h, int w, int max_points, int rmax, int n_sim);         // 0 for arguments the call refuses
int launch_droplet_points(const int* count, const int* area, const long long* sum_y, const long long* sum_x, int max_points,
                          const unsigned char* window, int h, int w, int* out_py, int* out_px, int* out_info,
                          hipStream_t stream);
int launch_ripley_counts(const int* py, const int* px, const int* n_points, int max_points, const unsigned char* window, int h,
                         int w, int rmax, int n_sim, unsigned seed, void* workspace, long workspace_bytes, int* out_n,
                         long long* out_pairs, long long* out_pairs_all, hipStream_t stream);

// boundary.hip: surface distances between the boundary pixels of two int32 label maps
long boundary_distances_workspace_bytes(int h, int w);      // 0 for a geometry the call refuses
int launch_boundary_distances(const int* label_a, int max_a, const int* label_b, int max_b, int h, int w, int radius,
                              void* workspace, long workspace_bytes, long long* hist, int* dmax, long long* out_a,
                              long long* out_b, hipStream_t stream);

// split.hip: exact squared Euclidean distance transform and the split of touching droplets (include/unetdc_hip.h)
int launch_edt_sq(const unsigned char* mask, int h, int w, int* out_d2, void* workspace, long workspace_bytes,
                  hipStream_t stream);
// the column pass alone, for boundary.hip: g[y][x] = the distance to the nearest zero pixel of column x, 0x7fffffff without one.
// No checks, no check_launch: the caller does both.
void launch_edt_col(const unsigned char* mask, int* g, int h, int w, hipStream_t stream);
long split_workspace_bytes(int h, int w);
int launch_split_stats(const unsigned char* mask, int h, int w, int min_area, int split_depth_half_px, void* workspace,
                       long workspace_bytes, int* out_count, int* out_area, long long* out_sumy, long long* out_sumx,
                       int* out_root, int* out_label, int max_out, hipStream_t stream);

// clean.hip: hysteresis threshold and hole filling of a {0,1} mask (include/unetdc_hip.h)
long mask_clean_workspace_bytes(int h, int w);
int launch_mask_clean(const unsigned char* strong, const unsigned char* weak, int h, int w, int max_hole_area, void* workspace,
                      long workspace_bytes, unsigned char* out_mask, int* out_counts, hipStream_t stream);

// diffmap.hip: the difference map of a predicted mask against an annotated one, and its 8-connected regions of equal class
// (include/unetdc_hip.h)
long diff_regions_workspace_bytes(int h, int w);            // 0 for a geometry the call refuses
int launch_diff_regions(const unsigned char* pred, const unsigned char* gt, int h, int w, int min_area, void* workspace,
                        long workspace_bytes, long long* out_image, int* out_count, int* out_class, int* out_area,
                        long long* out_sumy, long long* out_sumx, int* out_neighbors, int max_out, hipStream_t stream);
int launch_diff_paint(const unsigned char* pred, const unsigned char* gt, const unsigned char* rgb, int h, int w,
                      unsigned char* out_diff, unsigned char* out_overlay, hipStream_t stream);

// sweep.hip: the confusion matrix of the thresholded mask against an annotation at every threshold of a grid (DESIGN.md
// section 14; include/unetdc_hip.h)
int launch_thresh_sweep(const float* probs, int n, int ph, int pw, const unsigned char* gt, int oh, int ow, const int* xofs,
                        const short* xcoef, const int* yofs, const short* ycoef, int k, long long* hist, hipStream_t stream);

// tile.hip: overlapping network-size tiles of an image and the blend of their probabilities (DESIGN.md section 15;
// include/unetdc_hip.h)
int launch_tile_gather(const unsigned char* src, int h, int w, int cn, float* tiles, int t, const int* yo, int ny, const int* xo,
                       int nx, int t0, int count, hipStream_t stream);
int launch_tile_blend(const float* tiles, int t, int overlap, const int* yo, int ny, const int* xo, int nx, float* out, int h,
                      int w, hipStream_t stream);

// tta.hip: the D4 variants of a batch of square planes and the mean of the outputs mapped back (DESIGN.md section 17;
// include/unetdc_hip.h)
int launch_dihedral_expand(const float* x, int n, int c, int s, int nvar, float* out, hipStream_t stream);
int launch_dihedral_mean(const float* p, int n, int s, int nvar, float* out, hipStream_t stream);
int launch_dihedral_mean_env(const float* p, int n, int s, int nvar, float* out_mean, float* out_lo, float* out_hi,
                             hipStream_t stream);

// augment.hip: elastic displacement fields + the per-batch augmentation gather.  AugRecord is the layout of the public
// unetdc_augment_params (include/unetdc_hip.h; abi.hip asserts the two agree).
constexpr int AUG_HFLIP = 1, AUG_VFLIP = 2, AUG_BC = 4;
constexpr int AUG_MAX_SEEDS = 64;         // field slots per row/column-pass launch (seeds go by value in the kernel arguments)
constexpr int AUG_MAX_BATCH = 32;         // samples per gather launch (records go by value: 1 KB of kernel arguments)
struct AugRecord {
  int src, flags, k, field;
  float alpha, beta_max;
  int reserved[2];
};
long elastic_fields_workspace_bytes(int n, int h, int w, double sigma);
int launch_elastic_fields(const unsigned* seeds, int n, int h, int w, double sigma, float alpha, float* fields,
                          void* workspace, long workspace_bytes, hipStream_t stream);
int launch_augment_gather(const float* cache_img, const unsigned char* cache_mask, int ncache, int c, int h, int w,
                          const AugRecord* params, int n, const float* fields, int nfields, float* out_img, float* out_mask,
                          hipStream_t stream);

// crop.hip: random S x S windows of images cached at their own size, cut, scaled to [0, 1] and augmented in one pass (DESIGN.md
// section 16).  CropRecord is the layout of the public unetdc_crop_params and unetdc_crop_scaled_params (abi.hip asserts that
// the three agree).  t: the side of the source window of unetdc_crop_gather_scaled, which resamples it to S x S (scale
// jitter); unetdc_crop_gather does not read it (the public struct calls it `reserved`).
struct CropRecord {
  long long img_off, mask_off;
  int h, w, y0, x0, flags, k, field;
  float alpha, beta_max;
  int t;
};
// who: the entry point's name for the messages; scaled: the source window has side params[i].t, else s
int launch_crop_gather(const char* who, bool scaled, const unsigned char* images, long images_bytes, const unsigned char* masks,
                       long masks_bytes, int c, int s, const CropRecord* params, int n, const float* fields, int nfields,
                       float* out_img, float* out_mask, hipStream_t stream);

// preprocess.hip: rolling-ball correction + bilinear resize to the network input
long rolling_ball_workspace_bytes(int h, int w, int cn);
int launch_rolling_ball(const unsigned char* src, unsigned char* dst, int h, int w, int cn, int k, void* workspace,
                        long workspace_bytes, hipStream_t stream);
int launch_resize_linear_chw(const unsigned char* src, int h, int w, int cn, float* dst, int dh, int dw, const int* xofs,
                             const short* xa, const int* yofs, const short* ya, hipStream_t stream);
// erosion (is_max false) / dilation of a single-channel plane by the k x k rectangle (morph_kernel, outside pixels ignored)
int launch_morph_rect(const unsigned char* src, unsigned char* dst, int h, int w, int k, bool is_max, hipStream_t stream);

// window.hip: order statistics of a deep image by radix select, the integer window to 8 bits, the maximum over planes (DESIGN.md
// section 29; include/unetdc_hip.h)
long u16_ranks_workspace_bytes(int h, int w, int c, int nq);        // 0 for arguments the call refuses
int launch_u16_ranks(const unsigned short* src, int h, int w, int c, const int* ppm, int nq, void* workspace, long workspace_bytes,
                     int* out_value, int* out_below, int* out_equal, hipStream_t stream);
int launch_window_u16_to_u8(const unsigned short* src, int h, int w, int c, const int* levels, unsigned char* dst, int dc,
                            hipStream_t stream);
int launch_planes_max_u16(const unsigned short* src, int planes, int h, int w, unsigned short* dst, hipStream_t stream);

// density.hip: ROI, radial and spatial droplet density maps (include/unetdc_hip.h, unetdc_density_maps)
long density_workspace_bytes(int h, int w);
int launch_density_maps(const unsigned char* rgb, const unsigned char* mask, int h, int w, const int* dcount, const int* darea,
                        const long long* dsumy, const long long* dsumx, int dcap, int nb_layers, double sigma,
                        const double* taps, void* workspace, long workspace_bytes, unetdc_density_stats* stats,
                        unsigned char* radial_index, unsigned char* spatial_index, unsigned char* out_blur,
                        unsigned char* out_roi, unsigned char* out_ring, float* out_radial, float* out_spatial,
                        hipStream_t stream);
int launch_density_sqrt(const long long* x, double* out, long n, hipStream_t stream);

// loss.hip: wt = the per-pixel weight of the focal term ([nimg][hw]), null = the unweighted loss
long loss_workspace_bytes(int nimg, long hw);
int launch_loss_fwd(const float* p, const float* t, const float* wt, float* loss_out, float* coef, void* workspace,
                    long workspace_bytes, int nimg, long hw, float alpha, float gamma, float ratio, float smooth,
                    hipStream_t stream);
int launch_loss_bwd(const float* p, const float* t, const float* wt, const float* coef, const float* gout, float* dp, int nimg,
                    long hw, float alpha, float gamma, float ratio, hipStream_t stream);

// border.hip: the separation weight map of the border-weighted loss (include/unetdc_hip.h)
long border_workspace_bytes(int n, int h, int w, int radius);       // 0: a geometry the launcher refuses
int launch_border_weights(const float* target, int n, int h, int w, float w0, float sigma, int radius, float* out_weight,
                          int* out_d1, int* out_d2, void* workspace, long workspace_bytes, hipStream_t stream);

}  // namespace unetdc
