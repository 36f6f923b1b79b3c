// Surface distances between two int32 label maps: for every boundary pixel of one map the exact squared
// Euclidean distance to the nearest boundary pixel of the other, reduced on chip to a histogram of d^2 up to R^2 (+ "far"), the
// largest d^2 per direction and count / max / sum of d^2 per object.  All integer work, defined pixel by pixel: the record does
// not depend on the order in which anything runs (bitwise reproducible, equal to utils/droplet_boundary.py).
//
//   boundary_mark_kernel  one pass over both maps: nb[p] = 0 where p is a boundary pixel (a label in range with a 4-neighbour
//                         outside the image or of another value after the range rule), 1 elsewhere: the mask convention of
//                         edt_col_kernel.  Its first threads also initialise the per-object tables (0 / -1 / 0).
//                         The two planes lie side by side, row y of A then row y of B: ONE plane of width 2 w.
//   edt_col_kernel        (split.hip, unchanged) g[y][x] = the distance to the nearest boundary pixel of column x: one launch
//                         over the [h][2 w] plane serves both maps (the kernel is bound by the latency of its walk down and
//                         up a column, one wave per 64 columns: twice the columns take the same time)
//   boundary_row_kernel   edt_row_kernel's outward scan, evaluated ONLY at the query pixels (the boundary pixels of the other
//                         map); no D2 plane.  blockIdx.y is the direction; a workgroup strides over rows.  Per row: the query
//                         columns are compacted into an LDS list (ballot + prefix count, one LDS add per wave and 64 pixels); a
//                         row without queries ends there, after reading w bytes.  Else the row of g goes to LDS with the vote
//                         for "no finite column" (every query is UNETDC_EDT_INF), and the threads share the LIST, so the lanes
//                         of a wave all scan.  d^2 goes into the workgroup's LDS histogram, which lives across its rows and is
//                         flushed once (nonzero bins, 64-bit adds); the maximum stays in a register until one wave reduction
//                         and one atomicMax per wave; the per-object rows take one atomic triple per run of equal labels in
//                         a wave's part of the list (a one-label map would put every pixel on three addresses).
#include "kernels.h"
#include "wave_ops.h"

namespace unetdc {

constexpr int BOUNDARY_MAX_SIDE = 16384;          // d^2 <= 2 * 16383^2 < 2^29; a row of g and its query list fit the LDS
constexpr int BOUNDARY_MAX_RADIUS = 64;           // R^2 + 2 <= 4098 bins
constexpr int BOUNDARY_NONE = 0x7fffffff;         // edt_col_kernel's "no background in this column"
constexpr int BOUNDARY_ROW_GROUPS = 512;          // workgroups per direction: each flushes its histogram once

__device__ __forceinline__ int boundary_label(int v, int k) { return (v >= 1 && v <= k) ? v : 0; }

__device__ __forceinline__ unsigned char boundary_not(const int* __restrict__ L, int k, int i, int y, int x, int h, int w) {
  const int a = boundary_label(L[i], k);
  if (a == 0) return 1;
  if (y == 0 || x == 0 || y == h - 1 || x == w - 1) return 0;
  const bool edge = boundary_label(L[i - w], k) != a || boundary_label(L[i - 1], k) != a || boundary_label(L[i + 1], k) != a ||
                    boundary_label(L[i + w], k) != a;
  return edge ? 0 : 1;
}

__device__ __forceinline__ void boundary_table_init(long long* __restrict__ t, int k, int first, int stride) {
  if (!t) return;
  for (int j = first; j < k; j += stride) {
    t[j] = 0;
    t[(long)k + j] = -1;
    t[2l * k + j] = 0;
  }
}

__global__ __launch_bounds__(256) void boundary_mark_kernel(const int* __restrict__ la, int ka, const int* __restrict__ lb, int kb,
                                                            int h, int w, unsigned char* __restrict__ nb,
                                                            long long* __restrict__ out_a, long long* __restrict__ out_b) {
  const int n = h * w, first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  boundary_table_init(out_a, ka, first, stride);
  boundary_table_init(out_b, kb, first, stride);
  for (int i = first; i < n; i += stride) {
    const int y = i / w, x = i - y * w;
    const long o = (long)y * 2 * w + x;
    nb[o] = boundary_not(la, ka, i, y, x, h, w);
    nb[o + w] = boundary_not(lb, kb, i, y, x, h, w);
  }
}

struct BoundarySide {
  const unsigned char* nb;    // the queries: nb == 0; row y at nb + y * 2 w
  const int* g;               // column distances of the OTHER map; row y at g + y * 2 w
  const int* label;           // the map of the queries, for the per-object rows
  long long* table;           // [3][k] or null
  int k;
};

// dynamic LDS: row[w] int, bins[R^2 + 2] int, count[4] int (16 bytes), qx[w] unsigned short
static long boundary_row_lds(int w, int radius) { return 4l * w + 4l * (radius * radius + 2) + 16 + 2l * w; }

__global__ __launch_bounds__(256) void boundary_row_kernel(BoundarySide s0, BoundarySide s1, int h, int w, int radius,
                                                           unsigned long long* __restrict__ hist, int* __restrict__ dmax) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  const int dir = blockIdx.y;
  const BoundarySide s = dir ? s1 : s0;
  const int far = radius * radius + 1, nbins = far + 1;
  int* row = lds;
  int* bins = row + w;
  int* count = bins + nbins;
  unsigned short* qx = reinterpret_cast<unsigned short*>(count + 4);
  const int lane = threadIdx.x & 63;
  for (int b = threadIdx.x; b < nbins; b += 256) bins[b] = 0;
  int best_max = -1, turn = 0;
  for (int y = blockIdx.x; y < h; y += gridDim.x, turn ^= 1) {
    const long base = (long)y * w, prow = (long)y * 2 * w;
    int* nfound = count + turn;                             // two counters in turn: the one of the row before may still be read
    if (threadIdx.x == 0) *nfound = 0;
    __syncthreads();                                        // also: the row before is done with row[] and qx[]
    for (int x0 = threadIdx.x - lane; x0 < w; x0 += 256) {  // uniform per wave: the ballot needs all 64 lanes
      const int x = x0 + lane;
      const bool q = x < w && s.nb[prow + x] == 0;
      const unsigned long long m = __ballot(q);
      if (m == 0ull) continue;
      int at = 0;
      if (lane == 0) at = atomicAdd(nfound, __popcll(m));
      at = __shfl(at, 0, 64);
      if (q) qx[at + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)x;
    }
    __syncthreads();
    const int nq = *nfound;
    if (nq == 0) continue;                                  // uniform in the workgroup
    int finite = 0;
    for (int x = threadIdx.x; x < w; x += 256) {
      const int v = s.g[prow + x];
      row[x] = v;
      finite |= v != BOUNDARY_NONE;
    }
    const bool some = __syncthreads_or(finite);             // also the barrier that publishes row[]
    for (int j0 = threadIdx.x - lane; j0 < nq; j0 += 256) { // uniform per wave
      const int j = j0 + lane;
      const bool live = j < nq;
      int d2 = UNETDC_EDT_INF, x = 0;
      if (live) {
        x = qx[j];
        if (some) {
          const int g0 = row[x];
          int best = g0 == BOUNDARY_NONE ? UNETDC_EDT_INF : g0 * g0;
          for (int dx = 1; dx * dx < best; ++dx) {
            const int l = x - dx, r = x + dx, dd = dx * dx;
            if (l < 0 && r >= w) break;
            if (l >= 0) {
              const int v = row[l];
              if (v != BOUNDARY_NONE) best = min(best, dd + v * v);
            }
            if (r < w) {
              const int v = row[r];
              if (v != BOUNDARY_NONE) best = min(best, dd + v * v);
            }
          }
          d2 = best;
        }
        atomicAdd(&bins[min(d2, far)], 1);
        best_max = max(best_max, d2);
      }
      if (s.table) {                                        // uniform
        // One atomic triple per run of equal labels among the wave's 64 list entries (the list keeps the order of the row
        // within 64 pixels, so the two or three boundary pixels where a row crosses an outline sit next to each other, and a
        // one-label map is one run): wave_runs, then the run's maximum and sum (wave_ops.h).
        const int k = live ? s.label[base + x] : 0;         // a query's label is in range; the dead lanes form the last run
        const WaveRuns runs = wave_runs(k, lane);
        const int m = run_max(live ? d2 : -1, runs, lane);
        const long long t = run_sum(live ? (long long)d2 : 0ll, runs, lane);
        if (k != 0 && runs.head) {
          atomic_add64(s.table + k - 1, runs.len);
          atomicMax(s.table + s.k + k - 1, (long long)m);
          atomic_add64(s.table + 2l * s.k + k - 1, t);
        }
      }
    }
  }
  best_max = wave_max(best_max);
  if (lane == 0 && best_max >= 0) atomicMax(&dmax[dir], best_max);
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += 256) {
    const int c = bins[b];
    if (c) atomicAdd(&hist[(long)dir * nbins + b], (unsigned long long)c);
  }
}

// one int32 plane g and one uint8 plane nb of [h][2 w] each (row y of A, then row y of B), 64 spare bytes: 10 bytes per pixel
struct BoundaryPlanes {
  int* g;
  unsigned char* nb;
};
static Layout<BoundaryPlanes> boundary_layout(int h, int w, void* workspace) {
  if (!(h >= 1 && w >= 1 && h <= BOUNDARY_MAX_SIDE && w <= BOUNDARY_MAX_SIDE)) return {false, 0, {}};
  const long n = (long)h * w;
  Carver c(workspace);
  BoundaryPlanes p;
  p.g = c.take<int>(2 * n);
  p.nb = c.take<unsigned char>(2 * n);
  c.slack(64);
  return {true, c.bytes(), p};
}
long boundary_distances_workspace_bytes(int h, int w) { return boundary_layout(h, w, nullptr).bytes; }

int launch_boundary_distances(const int* label_a, int max_a, const int* label_b, int max_b, int h, int w, int radius,
                              void* workspace, long workspace_bytes, long long* hist, int* dmax, long long* out_a,
                              long long* out_b, hipStream_t stream) {
  UNETDC_REQUIRE(label_a && label_b && workspace && hist && dmax, "boundary_distances: null pointer");
  const auto lay = boundary_layout(h, w, workspace);
  UNETDC_REQUIRE(lay.ok && radius >= 1 && radius <= BOUNDARY_MAX_RADIUS && max_a >= 0 && max_b >= 0,
                 "boundary_distances: bad geometry (sides 1..16384, radius 1..64, non-negative label limits)");
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(hist) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(out_a) & 7) == 0 && (reinterpret_cast<uintptr_t>(out_b) & 7) == 0,
                 "boundary_distances: workspace must be 4-byte aligned, hist and the tables 8-byte aligned");
  if (int rc = require_workspace("boundary_distances", workspace_bytes, lay.bytes)) return rc;
  const int lds = (int)boundary_row_lds(w, radius);
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&boundary_row_kernel), lds, "boundary_row_kernel")) return rc;
  const auto [g, nb] = lay.planes;
  if (max_a == 0) out_a = nullptr;
  if (max_b == 0) out_b = nullptr;
  hipLaunchKernelGGL(boundary_mark_kernel, dim3(grid_for((long)h * w, 256, 4096)), dim3(256), 0, stream, label_a, max_a, label_b,
                     max_b, h, w, nb, out_a, out_b);
  launch_edt_col(nb, g, h, 2 * w, stream);
  const BoundarySide sa{nb, g + w, label_a, out_a, max_a}, sb{nb + w, g, label_b, out_b, max_b};
  hipLaunchKernelGGL(boundary_row_kernel, dim3(grid_for(h, 1, BOUNDARY_ROW_GROUPS), 2), dim3(256), (size_t)lds, stream, sa, sb, h,
                     w, radius, reinterpret_cast<unsigned long long*>(hist), dmax);
  return check_launch("boundary kernels");
}

}  // namespace unetdc
