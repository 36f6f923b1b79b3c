// Splitting touching droplets on the GPU ("Splitting touching droplets"): an exact squared Euclidean distance
// transform of the mask, ascent basins of that distance, and an order-free merge of neighbouring basins whose saddle lies
// less than the split depth below the lower of their two peaks.  All integer work, defined pixel by pixel, so the result
// does not depend on the order in which anything runs (bitwise reproducible, equal to utils/droplet_split.py).
//
//   edt_col_kernel    g[y][x] = distance to the nearest background pixel of column x (EDT_NONE when the column has none):
//                     one thread per column walks down, then up; neighbouring threads read neighbouring bytes
//   edt_row_kernel    D2[y][x] = min over x' of (x - x')^2 + g[y][x']^2: one workgroup per row, the row of g in LDS, every
//                     thread scans outward from x and stops once dx^2 >= the best so far (no x' further out can win).
//                     A mask without background (no finite g in the row, equally in every row) gets UNETDC_EDT_INF after one
//                     workgroup-wide vote, without any scan.
//   split_ascent      B[p] = the pixel with the largest key (D2, -index) among p and its foreground 4-neighbours
//   split_roots       B[p] = the end of p's pointer chain (keys strictly grow along it: no cycle); chains are compressed
//                     as they are walked, like ccl_stats_kernel compresses L
//   split_merge       for every foreground pair (p, right / down neighbour): same basin, or
//                     sqrt(min peak) - sqrt(min(D2[p], D2[q])) <= H2 / 2 in integers  ->  ccl_unite in the union-find L
//   launch_ccl_finish (ccl.hip) per-class sums, min_area, raster-order compaction;  launch_ccl_label: the int32 label map
#include "kernels.h"
#include "ccl_uf.h"

namespace unetdc {

constexpr int EDT_NONE = 0x7fffffff;              // g: no background pixel in this column
constexpr int SPLIT_MAX_SIDE = 16384;             // D2 <= 2 * 16383^2 < 2^29; one row of g fits 64 KiB of LDS

__global__ __launch_bounds__(64) void edt_col_kernel(const unsigned char* __restrict__ mask, int* __restrict__ g, int h, int w) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  int d = EDT_NONE;
#pragma unroll 8
  for (int y = 0; y < h; ++y) {
    const long i = (long)y * w + x;
    d = mask[i] ? (d == EDT_NONE ? EDT_NONE : d + 1) : 0;
    g[i] = d;
  }
  d = EDT_NONE;
#pragma unroll 8
  for (int y = h - 1; y >= 0; --y) {
    const long i = (long)y * w + x;
    d = mask[i] ? (d == EDT_NONE ? EDT_NONE : d + 1) : 0;
    if (d < g[i]) g[i] = d;
  }
}

__global__ __launch_bounds__(256) void edt_row_kernel(const int* __restrict__ g, int* __restrict__ d2, int w) {
  extern __shared__ int row[];
  const int* grow = g + (long)blockIdx.x * w;
  int* out = d2 + (long)blockIdx.x * w;
  int finite = 0;
  for (int x = threadIdx.x; x < w; x += 256) {
    const int v = grow[x];
    row[x] = v;
    finite |= v != EDT_NONE;
  }
  if (!__syncthreads_or(finite)) {                          // also the barrier that publishes row[]
    for (int x = threadIdx.x; x < w; x += 256) out[x] = UNETDC_EDT_INF;
    return;
  }
  for (int x = threadIdx.x; x < w; x += 256) {
    const int g0 = row[x];
    int best = g0 == EDT_NONE ? UNETDC_EDT_INF : g0 * g0;
    for (int dx = 1; dx * dx < best; ++dx) {
      const int l = x - dx, r = x + dx, dd = dx * dx;
      if (l < 0 && r >= w) break;
      if (l >= 0) {
        const int v = row[l];
        if (v != EDT_NONE) best = min(best, dd + v * v);
      }
      if (r < w) {
        const int v = row[r];
        if (v != EDT_NONE) best = min(best, dd + v * v);
      }
    }
    out[x] = best;
  }
}

__global__ void split_ascent_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ d2, int* __restrict__ B,
                                    int h, int w) {
  const int n = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int bi = i;
    if (mask[i]) {
      const int y = i / w, x = i - y * w;
      int bd = d2[i];
      // candidates in increasing index: a tie in D2 goes to the smaller index, so a later candidate needs a larger D2,
      // an earlier one (up, left: visited first) wins with an equal one
      if (y > 0 && mask[i - w]) { const int v = d2[i - w]; if (v >= bd) { bd = v; bi = i - w; } }
      if (x > 0 && mask[i - 1]) { const int v = d2[i - 1]; if (v > bd || (v == bd && bi == i)) { bd = v; bi = i - 1; } }
      if (x + 1 < w && mask[i + 1]) { const int v = d2[i + 1]; if (v > bd) { bd = v; bi = i + 1; } }
      if (y + 1 < h && mask[i + w]) { const int v = d2[i + w]; if (v > bd) { bd = v; bi = i + w; } }
    }
    B[i] = bi;
  }
}

__global__ void split_roots_kernel(const unsigned char* __restrict__ mask, int* __restrict__ B, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (!mask[i]) continue;
    // every value ever stored in B[i] lies on i's own chain, so a concurrent shortcut costs or saves hops, nothing else
    const int r = ccl_find(B, i);
    __hip_atomic_store(&B[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// unite iff sqrt(P) - sqrt(S) <= H2 / 2:  t = 4P - 4S - H2^2 <= 0, or t^2 <= 16 H2^2 S.  With t > 0: H2^2 < 4P < 2^31 and
// S < 2^29, so the right side stays below 2^64 and t^2 below 2^62.
__device__ __forceinline__ bool split_passes(int P, int S, long long h2sq) {
  const long long t = 4ll * P - 4ll * S - h2sq;
  if (t <= 0) return true;
  return (unsigned long long)t * (unsigned long long)t <= 16ull * (unsigned long long)h2sq * (unsigned long long)S;
}

__global__ void split_merge_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ d2, const int* __restrict__ B,
                                   int* __restrict__ L, int h, int w, long long h2sq) {
  const int n = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (!mask[i]) continue;
    const int y = i / w, x = i - y * w;
    const int bi = B[i], di = d2[i], pi = d2[bi];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int j = k == 0 ? i + 1 : i + w;
      if (k == 0 ? x + 1 >= w : y + 1 >= h) continue;
      if (!mask[j]) continue;
      const int bj = B[j];
      if (bi == bj || split_passes(min(pi, d2[bj]), min(di, d2[j]), h2sq)) ccl_unite(L, i, j);
    }
  }
}

static bool split_sides_ok(int h, int w) { return h > 0 && w > 0 && h <= SPLIT_MAX_SIDE && w <= SPLIT_MAX_SIDE; }

// split_stats: the ccl workspace with two more planes, D2 and B (B holds g during the distance transform)
static Layout<CclWorkspace> split_layout(int h, int w, void* workspace) {
  return split_sides_ok(h, w) ? ccl_layout(h, w, 2, workspace) : Layout<CclWorkspace>{};
}
long split_workspace_bytes(int h, int w) { return split_layout(h, w, nullptr).bytes; }

void launch_edt_col(const unsigned char* mask, int* g, int h, int w, hipStream_t stream) {
  hipLaunchKernelGGL(edt_col_kernel, dim3((w + 63) / 64), dim3(64), 0, stream, mask, g, h, w);
}

static void enqueue_edt(const unsigned char* mask, int h, int w, int* d2, int* g, hipStream_t stream) {
  launch_edt_col(mask, g, h, w, stream);
  hipLaunchKernelGGL(edt_row_kernel, dim3(h), dim3(256), (size_t)w * 4, stream, g, d2, w);
}

int launch_edt_sq(const unsigned char* mask, int h, int w, int* out_d2, void* workspace, long workspace_bytes,
                  hipStream_t stream) {
  UNETDC_REQUIRE(mask && out_d2 && workspace, "edt_sq: null pointer");
  UNETDC_REQUIRE(split_sides_ok(h, w), "edt_sq: bad geometry (sides 1..16384)");
  Carver c(workspace);                                      // one plane for g, 64 spare bytes (no query of its own)
  int* g = c.take<int>((long)h * w);
  c.slack(64);
  if (int rc = require_workspace("edt_sq", workspace_bytes, c.bytes())) return rc;
  enqueue_edt(mask, h, w, out_d2, g, stream);
  return check_launch("edt kernels");
}

int launch_split_stats(const unsigned char* mask, int h, int w, int min_area, int split_depth_half_px, void* workspace,
                       long workspace_bytes, int* out_count, int* out_area, long long* out_sumy, long long* out_sumx,
                       int* out_root, int* out_label, int max_out, hipStream_t stream) {
  UNETDC_REQUIRE(mask && workspace && out_count && out_area && out_sumy && out_sumx, "split_stats: null pointer");
  const auto lay = split_layout(h, w, workspace);
  UNETDC_REQUIRE(lay.ok && max_out >= 0, "split_stats: bad geometry (sides 1..16384)");
  UNETDC_REQUIRE(split_depth_half_px >= 0, "split_stats: negative split depth");
  if (int rc = require_workspace("split_stats", workspace_bytes, lay.bytes)) return rc;
  const int n = h * w, g = grid_for(n, 256, 4096);
  const CclPlanes& p = lay.planes.ccl;
  int *d2 = lay.planes.more, *B = d2 + n;
  // a depth at which every pair passes (H2 / 2 >= the largest possible sqrt(peak)) needs no more than that depth
  long long h2 = split_depth_half_px;
  if (h2 > 2ll * (h + w)) h2 = 2ll * (h + w);
  enqueue_edt(mask, h, w, d2, B, stream);
  launch_ccl_init(mask, p, n, stream);
  hipLaunchKernelGGL(split_ascent_kernel, dim3(g), dim3(256), 0, stream, mask, d2, B, h, w);
  hipLaunchKernelGGL(split_roots_kernel, dim3(g), dim3(256), 0, stream, mask, B, n);
  hipLaunchKernelGGL(split_merge_kernel, dim3(g), dim3(256), 0, stream, mask, d2, B, p.L, h, w, h2 * h2);
  // B is free again: it takes the rank of every kept class at its root pixel
  launch_ccl_finish(mask, h, w, min_area, p, out_count, out_area, out_sumy, out_sumx, out_root, out_label ? B : nullptr, max_out,
                    stream);
  if (out_label) launch_ccl_label(mask, p, B, min_area, out_label, n, stream);
  return check_launch("split kernels");
}

}  // namespace unetdc
