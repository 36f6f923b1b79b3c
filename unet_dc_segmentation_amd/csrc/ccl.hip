// Droplet quantification on the GPU: probabilities -> thresholded mask at the ORIGINAL image
// size -> 4-connected components -> per-droplet area / centroid sums, for
//   mask512 = (logits[i, 0].cpu().numpy() > thresh).astype(np.uint8)            /root/reference/quantify_droplets_batch.py:56
//   mask    = cv2.resize(mask512, (ow, oh), cv2.INTER_NEAREST)                                                     :57
//   lbl = label(bin_mask, connectivity=1); drop objects < min_area; lbl = label(lbl, connectivity=1)               :81-86
//   regionprops_table(lbl, ["label", "area", "equivalent_diameter", "centroid"])                                   :89-90
// What the reference's table needs from the device is, per kept droplet IN LABEL ORDER: its pixel count and the sums of
// its row / column coordinates (centroid = sums / area, equivalent_diameter = sqrt(4 area / pi): host, float64).
// skimage numbers the objects in raster order of their first pixel; a union-find whose root is the component's MINIMUM
// linear index gives exactly that order, and removing whole components does not change it.
//
//   mask_kernel      strict `>` on the fp32 probability (train_DC_focal.py:259 semantics), nearest-neighbour resize with
//                    cv2's index rule  src = min(floor(dst * src_size / dst_size), src_size - 1)
//   ccl_init/merge/compress   label equivalence by lock-free union-find (atomicMin towards the smaller root)
//   ccl_stats        integer atomics into per-root accumulators: exact and order-independent (bitwise reproducible)
//   ccl_count/scan/emit   roots with area >= min_area, compacted in increasing root order (three-level exclusive scan)
//   ccl_label        the int32 label map from the rank the emit kernel left at every kept root (unetdc_ccl_labels, split.hip)
// All byte / integer work: HBM-bound and tiny next to the network (a 512 x 512 mask is 256 KB).
#include "kernels.h"
#include "ccl_uf.h"
#include "linear_u8.h"
#include "wave_ops.h"

namespace unetdc {

__global__ void mask_kernel(const float* __restrict__ probs, int ph, int pw, float thresh, unsigned char* __restrict__ mask,
                            int oh, int ow, double fy, double fx) {
  const long n = (long)oh * ow;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / ow), x = (int)(i - (long)y * ow);
    int sy = (int)floor(y * fy), sx = (int)floor(x * fx);
    sy = sy < ph - 1 ? sy : ph - 1;
    sx = sx < pw - 1 ? sx : pw - 1;
    mask[i] = probs[(long)sy * pw + sx] > thresh ? 1 : 0;
  }
}

__global__ void ccl_init_kernel(const unsigned char* __restrict__ mask, int* __restrict__ L, int* __restrict__ area,
                                unsigned long long* __restrict__ sy, unsigned long long* __restrict__ sx, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    L[i] = i;
    area[i] = 0;
    sy[i] = 0ull;
    sx[i] = 0ull;
    (void)mask;
  }
}

__global__ void ccl_merge_kernel(const unsigned char* __restrict__ mask, int* __restrict__ L, int h, int w) {
  const int n = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (!mask[i]) continue;
    const int y = i / w, x = i - y * w;
    if (x + 1 < w && mask[i + 1]) ccl_unite(L, i, i + 1);   // 4-connectivity: right and down neighbours
    if (y + 1 < h && mask[i + w]) ccl_unite(L, i, i + w);
  }
}

__global__ void ccl_stats_kernel(const unsigned char* __restrict__ mask, int* __restrict__ L, int* __restrict__ area,
                                 unsigned long long* __restrict__ sy, unsigned long long* __restrict__ sx, int h, int w) {
  const int n = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (!mask[i]) continue;
    const int r = ccl_find(L, i);
    L[i] = r;                                               // path compression (a root keeps L[r] = r)
    const int y = i / w, x = i - y * w;
    atomicAdd(&area[r], 1);
    atomicAdd(&sy[r], (unsigned long long)y);
    atomicAdd(&sx[r], (unsigned long long)x);
  }
}

// kept[i] = pixel i is the root of a component with area >= min_area.  Three-level exclusive scan over 1024-element
// blocks (block sums -> one workgroup scans them -> emit), all in fixed order.
constexpr int CCL_BLK = 1024;

__device__ __forceinline__ bool ccl_kept(const unsigned char* mask, const int* L, const int* area, int i, int min_area) {
  return mask[i] && L[i] == i && area[i] >= min_area;
}

__global__ __launch_bounds__(256) void ccl_count_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ L,
                                                        const int* __restrict__ area, int n, int min_area,
                                                        int* __restrict__ blocksum) {
  __shared__ int red[4];
  const int b = blockIdx.x, base = b * CCL_BLK;
  int c = 0;
  for (int k = threadIdx.x; k < CCL_BLK; k += 256) {
    const int i = base + k;
    if (i < n && ccl_kept(mask, L, area, i, min_area)) ++c;
  }
  c = block_sum<256>(c, red);
  if (threadIdx.x == 0) blocksum[b] = c;
}

// one workgroup: the exclusive scan of the block sums in place (at most 2^20 of them, 1024 a trip); their sum is below 2^30
__global__ __launch_bounds__(1024) void ccl_scan_kernel(int* blocksum, int nblocks, int* __restrict__ total) {
  __shared__ int s_w[16];
  const long long sum = scan_plane(blocksum, blocksum, nblocks, s_w);
  if (threadIdx.x == 0) *total = (int)sum;
}

__global__ __launch_bounds__(256) void ccl_emit_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ L,
                                                       const int* __restrict__ area, const unsigned long long* __restrict__ sy,
                                                       const unsigned long long* __restrict__ sx, int n, int min_area,
                                                       const int* __restrict__ blockoff, int max_out, int* __restrict__ out_area,
                                                       long long* __restrict__ out_sy, long long* __restrict__ out_sx,
                                                       int* __restrict__ out_root, int* __restrict__ rank_of_root) {
  // thread 0..255 handle 4 consecutive pixels each and a block-level exclusive scan of the 256 per-thread counts gives every
  // kept root its rank
  __shared__ int s_w[4];
  const int b = blockIdx.x, base = b * CCL_BLK + threadIdx.x * 4;
  bool k[4];
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = base + j;
    k[j] = i < n && ccl_kept(mask, L, area, i, min_area);
    c += k[j] ? 1 : 0;
  }
  int rank = blockoff[b] + block_excl_scan<256>(c, s_w);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!k[j]) continue;
    const int i = base + j;
    if (rank < max_out) {
      out_area[rank] = area[i];
      out_sy[rank] = (long long)sy[i];
      out_sx[rank] = (long long)sx[i];
      if (out_root) out_root[rank] = i;
    }
    ++rank;
    if (rank_of_root) rank_of_root[i] = rank;               // 1-based, also past max_out (split.hip's label map)
  }
}

// label[i] = the 1-based output rank of pixel i's class, 0 on background and on classes below min_area
__global__ void ccl_label_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ L, const int* __restrict__ area,
                                 const int* __restrict__ rank_of_root, int min_area, int* __restrict__ label, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int v = 0;
    if (mask[i]) {
      const int r = L[i];                                   // compressed by ccl_stats_kernel
      if (area[r] >= min_area) v = rank_of_root[r];
    }
    label[i] = v;
  }
}

int launch_mask_from_probs(const float* probs, int ph, int pw, float thresh, unsigned char* mask, int oh, int ow,
                           hipStream_t stream) {
  UNETDC_REQUIRE(probs && mask && ph > 0 && pw > 0 && oh > 0 && ow > 0, "mask_from_probs: bad arguments");
  // cv2.resize(..., INTER_NEAREST): x_ofs[x] = min(cvFloor(x * (src_w / dst_w)), src_w - 1) in double precision
  hipLaunchKernelGGL(mask_kernel, dim3(grid_for((long)oh * ow, 256, 4096)), dim3(256), 0, stream, probs, ph, pw, thresh, mask, oh,
                     ow, (double)ph / (double)oh, (double)pw / (double)ow);
  return check_launch("mask_kernel");
}

// The reference calls cv2.resize(mask512, (ow, oh), cv2.INTER_NEAREST) (quantify_droplets_batch.py:57): the third positional
// parameter of cv2.resize is `dst`, so the flag is ignored and OpenCV's default 8-bit INTER_LINEAR runs on the {0,1} mask:
//   r = m[x0] * a0 + m[x1] * a1 (11-bit coefficients), then the vertical pass of linear_u8_combine (linear_u8.h): v in {0,1}
// Same tables as unetdc_resize_linear_u8_to_chw_f32 (utils/data_loader.py:linear_tables + the edge rule).
__global__ void mask_linear_kernel(const float* __restrict__ probs, int ph, int pw, float thresh, unsigned char* __restrict__ mask,
                                   int oh, int ow, const int* __restrict__ xofs, const short* __restrict__ xa,
                                   const int* __restrict__ yofs, const short* __restrict__ ya) {
  const long n = (long)oh * ow;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int dy = (int)(i / ow), dx = (int)(i - (long)dy * ow);
    const LinearTaps t = linear_u8_taps(xofs, xa, yofs, ya, dx, dy, pw, ph);
    const int m00 = probs[(long)t.sy0 * pw + t.sx0] > thresh, m01 = probs[(long)t.sy0 * pw + t.sx1] > thresh;
    const int m10 = probs[(long)t.sy1 * pw + t.sx0] > thresh, m11 = probs[(long)t.sy1 * pw + t.sx1] > thresh;
    const int v = linear_u8_combine(m00, m01, m10, m11, t.a0, t.a1, t.b0, t.b1);
    mask[i] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

int launch_mask_from_probs_linear(const float* probs, int ph, int pw, float thresh, unsigned char* mask, int oh, int ow,
                                  const int* xofs, const short* xcoef, const int* yofs, const short* ycoef, hipStream_t stream) {
  UNETDC_REQUIRE(probs && mask && xofs && xcoef && yofs && ycoef && ph > 0 && pw > 0 && oh > 0 && ow > 0,
                 "mask_from_probs_linear: bad arguments");
  hipLaunchKernelGGL(mask_linear_kernel, dim3(grid_for((long)oh * ow, 256, 4096)), dim3(256), 0, stream, probs, ph, pw, thresh, mask,
                     oh, ow, xofs, xcoef, yofs, ycoef);
  return check_launch("mask_linear_kernel");
}

// the two coordinate sums, the union-find, the areas, one block sum per CCL_BLK pixels (+ 16 words), one after the other
// without padding, and 64 spare bytes; `extra` > 0: from the next multiple of 64 that many more planes, 64 spare bytes again
Layout<CclWorkspace> ccl_layout(int h, int w, int extra, void* workspace) {
  if (!(h > 0 && w > 0 && (long)h * w < (1L << 30))) return {false, 0, {}};
  const long n = (long)h * w, nb = (n + CCL_BLK - 1) / CCL_BLK;
  Carver c(workspace);
  CclWorkspace p = {};
  p.ccl.sy = c.take<unsigned long long>(n);
  p.ccl.sx = c.take<unsigned long long>(n);
  p.ccl.L = c.take<int>(n);
  p.ccl.area = c.take<int>(n);
  p.ccl.blocksum = c.take<int>(nb + 16);
  c.slack(64);
  if (extra > 0) {
    c.align(64);
    p.more = c.take<int>(extra * n);
    c.slack(64);
  }
  return {true, c.bytes(), p};
}
long ccl_workspace_bytes(int h, int w) { return ccl_layout(h, w, 0, nullptr).bytes; }
long ccl_labels_workspace_bytes(int h, int w) { return ccl_layout(h, w, 1, nullptr).bytes; }

void launch_ccl_init(const unsigned char* mask, const CclPlanes& p, int n, hipStream_t stream) {
  hipLaunchKernelGGL(ccl_init_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, mask, p.L, p.area, p.sy, p.sx, n);
}

void launch_ccl_scan(int* blocksum, int nblocks, int* total, hipStream_t stream) {
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, stream, blocksum, nblocks, total);
}

void launch_ccl_finish(const unsigned char* mask, int h, int w, int min_area, const CclPlanes& p, int* out_count,
                       int* out_area, long long* out_sumy, long long* out_sumx, int* out_root, int* rank_of_root, int max_out,
                       hipStream_t stream) {
  const int n = h * w, nb = (n + CCL_BLK - 1) / CCL_BLK, g = grid_for(n, 256, 4096);
  hipLaunchKernelGGL(ccl_stats_kernel, dim3(g), dim3(256), 0, stream, mask, p.L, p.area, p.sy, p.sx, h, w);
  hipLaunchKernelGGL(ccl_count_kernel, dim3(nb), dim3(256), 0, stream, mask, p.L, p.area, n, min_area, p.blocksum);
  launch_ccl_scan(p.blocksum, nb, out_count, stream);
  hipLaunchKernelGGL(ccl_emit_kernel, dim3(nb), dim3(256), 0, stream, mask, p.L, p.area, p.sy, p.sx, n, min_area, p.blocksum,
                     max_out, out_area, out_sumy, out_sumx, out_root, rank_of_root);
}

void launch_ccl_label(const unsigned char* mask, const CclPlanes& p, const int* rank_of_root, int min_area, int* label, int n,
                      hipStream_t stream) {
  hipLaunchKernelGGL(ccl_label_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, mask, p.L, p.area, rank_of_root, min_area,
                     label, n);
}

int launch_ccl(const char* who, const unsigned char* mask, int h, int w, int min_area, void* workspace, long workspace_bytes,
               int* out_count, int* out_area, long long* out_sumy, long long* out_sumx, int* out_root, int* out_label,
               int max_out, hipStream_t stream) {
  UNETDC_REQUIRE(mask && workspace && out_count && out_area && out_sumy && out_sumx, "%s: null pointer", who);
  const auto lay = ccl_layout(h, w, out_label ? 1 : 0, workspace);     // labels: the rank of every kept component at its root
  UNETDC_REQUIRE(lay.ok && max_out >= 0, "%s: bad geometry", who);
  if (int rc = require_workspace(who, workspace_bytes, lay.bytes)) return rc;
  const int n = h * w, nb = (n + CCL_BLK - 1) / CCL_BLK;
  UNETDC_REQUIRE(nb <= 1024 * 1024, "%s: image too large", who);
  const CclPlanes& p = lay.planes.ccl;
  launch_ccl_init(mask, p, n, stream);
  hipLaunchKernelGGL(ccl_merge_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, mask, p.L, h, w);
  launch_ccl_finish(mask, h, w, min_area, p, out_count, out_area, out_sumy, out_sumx, out_root, lay.planes.more, max_out, stream);
  if (out_label) launch_ccl_label(mask, p, lay.planes.more, min_area, out_label, n, stream);
  return check_launch(out_label ? "ccl label kernels" : "ccl kernels");
}

}  // namespace unetdc
