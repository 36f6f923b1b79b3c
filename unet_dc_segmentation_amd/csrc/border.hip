// Separation weight map of the border-weighted loss: for every background pixel of a batch of masks the
// squared distances D1, D2 to the nearest and to the second-nearest 4-connected component inside the (2R + 1)^2 window, and
//   w = 1 + w0 * exp(-(sqrt(D1) + sqrt(D2))^2 / (2 sigma^2))  where D2 <= R^2,   w = 1 everywhere else.
// All integer work up to the last line, defined pixel by pixel: the planes are bitwise reproducible and equal to
// utils/border_weights.py.
//
//   border_init     L[i] = the first pixel of i's horizontal run inside its 64-pixel segment on foreground (target > 0.5), -1 on
//                   background; indices are local to the image
//   border_merge    ccl_unite (ccl_uf.h) of a run with the one before its segment and of the first vertical pair of every
//                   overlap of two runs, never across an image boundary
//   border_flatten  L[i] = its root: the component id of the passes below (unique per component within an image)
//   border_col      per pixel the two candidates of its column within |dy| <= R: the nearest foreground pixel (dy1, a) and
//                   the nearest one whose id differs from a (dy2, b).  16 x 64 tiles, the ids with an R-row halo in LDS, every
//                   pixel scans outward and stops at its second candidate; a tile without foreground in reach writes "none"
//   border_row      per background pixel the best two of distinct ids among (dx^2 + dy1^2, a), (dx^2 + dy2^2, b) over
//                   |dx| <= R: 2 x 128 pixel strips, the records with an R-column halo in LDS, outward scan that stops once
//                   dx^2 >= D2 (nothing further out can change the pair); foreground pixels and strips whose records are
//                   all "none" skip the scan
#include "kernels.h"
#include "ccl_uf.h"

namespace unetdc {

constexpr int BORDER_MAX_SIDE = 16384;
constexpr int BORDER_MAX_RADIUS = 64;
constexpr int BORDER_NONE = 0xff;                 // dy of a missing column candidate (dy <= 64 otherwise)
constexpr int BORDER_CT = 64, BORDER_CH = 16;     // border_col: tile width and rows
constexpr int BORDER_RW = 128, BORDER_RH = 2;     // border_row: strip width and rows

// A wave owns 64 consecutive pixels (linear index, BORDER_SEG-aligned: the grid strides are multiples of 256).  A foreground
// pixel starts as a child of the first pixel of its horizontal run inside that segment and its row (one ballot, no memory
// traffic): the union-find then only has to join runs, not pixels.
constexpr int BORDER_SEG = 64;

__global__ __launch_bounds__(256) void border_init_kernel(const float* __restrict__ target, int* __restrict__ L, int hw, int w) {
  const long base = (long)blockIdx.y * hw;
  const int lane = threadIdx.x & 63;
  for (int i0 = blockIdx.x * 256 + (threadIdx.x - lane); i0 < hw; i0 += gridDim.x * 256) {    // uniform per wave
    const int i = i0 + lane;
    const bool valid = i < hw;
    const bool fg = valid && target[base + i] > 0.5f;
    const unsigned long long zero = __ballot(!fg), rowstart = __ballot(valid && i % w == 0);
    if (!valid) continue;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long zb = zero & below, rs = rowstart & ((below << 1) | 1ull);
    const int a = zb ? 64 - __clzll((long long)zb) : 0;     // the lane behind the last background lane before this one
    const int b = rs ? 63 - __clzll((long long)rs) : 0;     // the last lane up to this one that starts a row
    L[base + i] = fg ? i0 + max(a, b) : -1;
  }
}

// Joins the runs: a run with the one that ends just before its segment, and vertically adjacent pixels.  A vertical pair whose
// left neighbours are a vertical foreground pair too is implied by that pair and the two runs, so only the first pair of every
// overlap of two runs is united.
__global__ __launch_bounds__(256) void border_merge_kernel(int* __restrict__ L, int h, int w) {
  const int hw = h * w;
  int* Li = L + (long)blockIdx.y * hw;
  // foreground entries are never negative, background entries are never written: a test of the sign is race free
  auto fg = [&](int j) { return __hip_atomic_load(&Li[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0; };
  for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
    if (!fg(i)) continue;
    const int y = i / w, x = i - y * w;
    if (x > 0 && (i & (BORDER_SEG - 1)) == 0 && fg(i - 1)) ccl_unite(Li, i - 1, i);
    if (y + 1 < h && fg(i + w) && !(x > 0 && fg(i - 1) && fg(i + w - 1))) ccl_unite(Li, i, i + w);
  }
}

__global__ void border_flatten_kernel(int* __restrict__ L, int hw) {
  int* Li = L + (long)blockIdx.y * hw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
    if (__hip_atomic_load(&Li[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
    // every value ever stored in L[i] lies on i's own chain (split_roots_kernel): a concurrent shortcut costs or saves hops
    const int r = ccl_find(Li, i);
    __hip_atomic_store(&Li[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// column record of a pixel: ids a, b (-1: none) and dy1 | dy2 << 8 (BORDER_NONE: none)
__global__ __launch_bounds__(256) void border_col_kernel(const int* __restrict__ L, int* __restrict__ ca, int* __restrict__ cb,
                                                         unsigned short* __restrict__ cd, int h, int w, int R) {
  extern __shared__ int lab[];                              // [BORDER_CH + 2 R][BORDER_CT]
  const int x0 = blockIdx.x * BORDER_CT, y0 = blockIdx.y * BORDER_CH;
  const long base = (long)blockIdx.z * h * w;
  const int rows = BORDER_CH + 2 * R;
  int any = 0;
  for (int i = threadIdx.x; i < rows * BORDER_CT; i += 256) {
    const int y = y0 - R + (i >> 6), x = x0 + (i & 63);
    const int v = (y >= 0 && y < h && x < w) ? L[base + (long)y * w + x] : -1;
    lab[i] = v;
    any |= v >= 0;
  }
  const bool some = __syncthreads_or(any);                  // also the barrier that publishes lab[]
  const int c = threadIdx.x & 63, x = x0 + c;
  if (x >= w) return;
  for (int r = threadIdx.x >> 6; r < BORDER_CH; r += 4) {
    const int y = y0 + r;
    if (y >= h) break;
    int a = -1, b = -1, d1 = BORDER_NONE, d2 = BORDER_NONE;
    if (some) {
      const int* col = lab + (r + R) * BORDER_CT + c;
      a = col[0];
      if (a >= 0) d1 = 0;
      for (int dy = 1; dy <= R; ++dy) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int v = col[(k ? dy : -dy) * BORDER_CT];
          if (v < 0) continue;
          if (a < 0) { a = v; d1 = dy; }
          else if (v != a && b < 0) { b = v; d2 = dy; }
        }
        if (b >= 0) break;
      }
    }
    const long i = base + (long)y * w + x;
    ca[i] = a;
    cb[i] = b;
    cd[i] = (unsigned short)(d1 | (d2 << 8));
  }
}

// (d, l) into the running best two of distinct ids (d1, l1), (d2, l2)
__device__ __forceinline__ void border_insert(int d, int l, int& d1, int& l1, int& d2, int& l2) {
  if (l == l1) { d1 = min(d1, d); }
  else if (d < d1) { d2 = d1; l2 = l1; d1 = d; l1 = l; }
  else if (l == l2) { d2 = min(d2, d); }
  else if (d < d2) { d2 = d; l2 = l; }
}

__global__ __launch_bounds__(256) void border_row_kernel(const int* __restrict__ ca, const int* __restrict__ cb,
                                                         const unsigned short* __restrict__ cd, float* __restrict__ out_w,
                                                         int* __restrict__ out_d1, int* __restrict__ out_d2, int h, int w, int R,
                                                         double w0, double two_sigma_sq) {
  __shared__ int sa[BORDER_RH][BORDER_RW + 2 * BORDER_MAX_RADIUS], sb[BORDER_RH][BORDER_RW + 2 * BORDER_MAX_RADIUS];
  __shared__ unsigned short sd[BORDER_RH][BORDER_RW + 2 * BORDER_MAX_RADIUS];
  const int tx = threadIdx.x & (BORDER_RW - 1), ty = threadIdx.x >> 7;
  const int x0 = blockIdx.x * BORDER_RW, y = blockIdx.y * BORDER_RH + ty;
  const long base = (long)blockIdx.z * h * w + (long)y * w;
  int any = 0;
  for (int i = tx; i < BORDER_RW + 2 * R; i += BORDER_RW) {
    const int x = x0 - R + i;
    int a = -1, b = -1, d = BORDER_NONE | (BORDER_NONE << 8);
    if (y < h && x >= 0 && x < w) { a = ca[base + x]; b = cb[base + x]; d = cd[base + x]; }
    sa[ty][i] = a; sb[ty][i] = b; sd[ty][i] = (unsigned short)d;
    any |= a >= 0;
  }
  const bool some = __syncthreads_or(any);                  // also the barrier that publishes the records
  const int x = x0 + tx;
  if (y >= h || x >= w) return;
  int D1 = UNETDC_EDT_INF, D2 = UNETDC_EDT_INF;
  if (some) {
    const int c = tx + R;
    if ((sd[ty][c] & 0xff) == 0) {
      D1 = D2 = 0;                                          // foreground
    } else {
      int l1 = -1, l2 = -1;
      for (int dx = 0; dx <= R; ++dx) {
        const int dd = dx * dx;
        if (dd >= D2) break;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (k && dx == 0) continue;
          const int i = k ? c - dx : c + dx;
          const int d = sd[ty][i], e1 = d & 0xff, e2 = d >> 8;
          if (e1 == BORDER_NONE) continue;                  // (then there is no second candidate either)
          // a candidate that is not below D2 changes nothing in any of the four cases
          const int da = dd + e1 * e1, db = dd + e2 * e2;
          if (da < D2) border_insert(da, sa[ty][i], D1, l1, D2, l2);
          if (e2 != BORDER_NONE && db < D2) border_insert(db, sb[ty][i], D1, l1, D2, l2);
        }
      }
    }
  }
  float wv = 1.f;
  if (D1 > 0 && D2 <= R * R) {
    // the arithmetic of the definition (utils/border_weights.py:weights_from_planes): fp64, every operation rounded on its own
    // (no contraction into an FMA), the weight rounded to fp32 once
    const double s = __dadd_rn(sqrt((double)D1), sqrt((double)D2));
    wv = (float)__dadd_rn(1.0, __dmul_rn(w0, exp(-__dmul_rn(s, s) / two_sigma_sq)));
  }
  out_w[base + x] = wv;
  if (out_d1) out_d1[base + x] = D1;
  if (out_d2) out_d2[base + x] = D2;
}

// ids, the two candidate ids (int32 each) and the packed dy pair (uint16) of every pixel, 64 spare bytes
struct BorderPlanes {
  int *L, *ca, *cb;
  unsigned short* cd;
};
static Layout<BorderPlanes> border_layout(int n, int h, int w, int radius, void* workspace) {
  if (!(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && h <= BORDER_MAX_SIDE && w <= BORDER_MAX_SIDE && (long)h * w < (1L << 30) &&
        radius >= 1 && radius <= BORDER_MAX_RADIUS))
    return {false, 0, {}};
  const long total = (long)n * h * w;
  Carver c(workspace);
  BorderPlanes p;
  p.L = c.take<int>(total);
  p.ca = c.take<int>(total);
  p.cb = c.take<int>(total);
  p.cd = c.take<unsigned short>(total);
  c.slack(64);
  return {true, c.bytes(), p};
}
long border_workspace_bytes(int n, int h, int w, int radius) { return border_layout(n, h, w, radius, nullptr).bytes; }

int launch_border_weights(const float* target, int n, int h, int w, float w0, float sigma, int radius, float* out_weight,
                          int* out_d1, int* out_d2, void* workspace, long workspace_bytes, hipStream_t stream) {
  UNETDC_REQUIRE(target && out_weight && workspace, "border_weights: null pointer");
  const auto lay = border_layout(n, h, w, radius, workspace);
  UNETDC_REQUIRE(lay.ok,
                 "border_weights: bad geometry (n 1..65535, sides 1..16384, h * w < 2^30, radius 1..64)");
  UNETDC_REQUIRE(sigma > 0.f && sigma <= 3.0e38f && w0 >= 0.f && w0 <= 3.0e38f,
                 "border_weights: sigma must be positive and w0 non-negative (both finite)");
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "border_weights: workspace must be 4-byte aligned");
  if (int rc = require_workspace("border_weights", workspace_bytes, lay.bytes)) return rc;
  const int hw = h * w;
  const auto [L, ca, cb, cd] = lay.planes;
  const dim3 flat(grid_for(hw, 256, 4096), n);
  hipLaunchKernelGGL(border_init_kernel, flat, dim3(256), 0, stream, target, L, hw, w);
  hipLaunchKernelGGL(border_merge_kernel, flat, dim3(256), 0, stream, L, h, w);
  hipLaunchKernelGGL(border_flatten_kernel, flat, dim3(256), 0, stream, L, hw);
  hipLaunchKernelGGL(border_col_kernel, dim3((w + BORDER_CT - 1) / BORDER_CT, (h + BORDER_CH - 1) / BORDER_CH, n), dim3(256),
                     (size_t)(BORDER_CH + 2 * radius) * BORDER_CT * 4, stream, L, ca, cb, cd, h, w, radius);
  hipLaunchKernelGGL(border_row_kernel, dim3((w + BORDER_RW - 1) / BORDER_RW, (h + BORDER_RH - 1) / BORDER_RH, n), dim3(256), 0,
                     stream, ca, cb, cd, out_weight, out_d1, out_d2, h, w, radius, (double)w0,
                     2.0 * ((double)sigma * (double)sigma));
  return check_launch("border kernels");
}

}  // namespace unetdc
