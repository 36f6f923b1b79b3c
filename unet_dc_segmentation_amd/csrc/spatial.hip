// Ripley's K of the droplet centroids with a Monte Carlo envelope of complete spatial randomness: the
// centroid pixels of a droplet table, and for the observed pattern and S simulated ones in the same window the counts n[r],
// pairs[r] (border-corrected) and pairs_all[r], r = 0..R.  Integer work only, sums of integers by atomics: the order in which
// anything runs does not show, two runs give the same bytes.  The host restatement is utils/spatial_stats.py.
//
//   spatial_points_kernel           ONE workgroup walks the table in chunks of 256: centroid rounded half up, kept when the window
//                           holds it; ballots and a four-wave prefix keep table order.  Writes N, n_dropped, the flag, and A
//                           without a window.
//   spatial_window_count_kernel     A = the nonzero pixels of the window (block sums, one atomic per workgroup)
//   spatial_window_rows_kernel      one wave per row: per 64-pixel block the ballot of its pixels (bits) and the count of the row's
//                           pixels before it (blkpre), a running sum down the row; the row's total
//   spatial_window_scan_kernel      ONE workgroup: rowpre[y] = the window's pixels in the rows above y, rowpre[h] = A.  Raster order is
//                           part of the contract, so both prefix planes come from scans, never from atomics.
//   spatial_sets_kernel      one thread per point of every set: set 0 copies the given points, set s + 1 draws point k as the
//                           t-th pixel of the window, t = mulhi64(u, A), u from the counter hash of (seed, s, k): two binary
//                           searches (rows, blocks of the row) and a select of the t-th set bit in one 64-pixel block; without
//                           a window t -> (t / w, t % w).  Then e = the largest r <= R with r^2 < min(D2_W, m^2); without a
//                           window no plane is read.
//   spatial_eligible_kernel  one workgroup per set: histogram of e in LDS -> n[r] = #{e >= r}; zeroes the set's pair counts
//   spatial_pairs_kernel     the hot path.  Point set = blockIdx.y.  The j points are staged in LDS in tiles of RIPLEY_TILE packed
//                           words; a wave owns one i at a time, its lanes run over the tile and histogram c(i, j) <= R into the
//                           wave's R + 1 LDS bins.  After the last tile the wave scans its bins inclusively; lane l keeps the
//                           running sums of the bins l, l + 64, ... in registers (pairs where r <= e(i), pairs_all everywhere).
//                           At the end the four waves meet in the workgroup's 64-bit LDS accumulators and the workgroup
//                           flushes once with 64-bit global atomics.  Nothing waits for another workgroup.
#include "hash32.h"
#include "kernels.h"
#include "wave_ops.h"
#include "workspace.h"

namespace unetdc {

constexpr int RIPLEY_MAX_R = 256, RIPLEY_MAX_SIMS = 999, RIPLEY_MAX_POINTS = 1 << 20;
constexpr int RIPLEY_TILE = 2048;                              // packed points per LDS tile (8 KiB)
constexpr int RIPLEY_CHUNKS = (RIPLEY_MAX_R + 1 + 63) / 64;    // bins per lane in the scan
constexpr unsigned RIPLEY_GOLDEN = 0x9E3779B9u;

struct RipleyPlanes {
  unsigned long long* bits;    // [h][nb] the window's pixels of one 64-pixel block, bit = column within the block
  unsigned* pts;               // [(1 + S)][max_points] (y << 16) | x
  int* e;                      // [(1 + S)][max_points]
  int* d2;                     // [h][w] D2_W
  int* g;                      // [h][w] + 64 bytes: the distance transform's own plane
  int* rowpre;                 // [h + 1]
  int* blkpre;                 // [h][nb]
  long g_bytes;
};

static Layout<RipleyPlanes> ripley_layout(int h, int w, int max_points, int rmax, int n_sim, void* workspace) {
  if (!(h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30) && max_points >= 1 &&
        max_points <= RIPLEY_MAX_POINTS && rmax >= 1 && rmax <= RIPLEY_MAX_R && n_sim >= 0 && n_sim <= RIPLEY_MAX_SIMS))
    return {false, 0, {}};
  const long nb = (w + 63) / 64, sets = 1 + n_sim;
  Carver c(workspace);
  RipleyPlanes p;
  p.bits = c.take<unsigned long long>((long)h * nb, 64);
  p.pts = c.take<unsigned>(sets * max_points, 64);
  p.e = c.take<int>(sets * max_points, 64);
  p.d2 = c.take<int>((long)h * w, 64);
  const long before = c.bytes();
  p.g = c.take<int>((long)h * w);
  c.slack(64);
  c.align(64);
  p.g_bytes = c.bytes() - before;
  p.rowpre = c.take<int>((long)h + 1, 64);
  p.blkpre = c.take<int>((long)h * nb, 64);
  return {true, c.bytes(), p};
}
long ripley_workspace_bytes(int h, int w, int max_points, int rmax, int n_sim) {
  return ripley_layout(h, w, max_points, rmax, n_sim, nullptr).bytes;
}

// ---- the droplet table -> points ----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void spatial_points_kernel(const int* __restrict__ count, const int* __restrict__ area,
                                                     const long long* __restrict__ sum_y, const long long* __restrict__ sum_x,
                                                     int max_points, const unsigned char* __restrict__ window, int h, int w,
                                                     int* __restrict__ out_py, int* __restrict__ out_px, int* __restrict__ out_info) {
  __shared__ int wave_n[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int total = *count;
  const int n = total < 0 ? 0 : total < max_points ? total : max_points;
  int kept = 0;                                                // uniform over the workgroup
  for (int base = 0; base < n; base += 256) {
    const int k = base + threadIdx.x;
    bool keep = false;
    int y = 0, x = 0;
    if (k < n) {
      const long long a = area[k] > 1 ? area[k] : 1;
      const long long yy = (2 * sum_y[k] + a) / (2 * a), xx = (2 * sum_x[k] + a) / (2 * a);
      if (sum_y[k] >= 0 && sum_x[k] >= 0 && yy < h && xx < w) {             // a point outside the image is outside the window
        y = (int)yy;
        x = (int)xx;
        keep = !window || window[(long)y * w + x] != 0;
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int at = kept + __popcll(m & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) at += wave_n[v];
    if (keep) {
      out_py[at] = y;
      out_px[at] = x;
    }
    kept += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out_info[0] = kept;
    out_info[1] = n - kept;
    out_info[2] = window ? 0 : h * w;
    out_info[3] = total > max_points ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void spatial_window_count_kernel(const unsigned char* __restrict__ window, int n, int* __restrict__ out_a) {
  __shared__ int part[4];
  int c = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) c += window[i] != 0;
  const int s = block_sum<256>(c, part);
  if (threadIdx.x == 0 && s) atomicAdd(out_a, s);
}

int launch_droplet_points(const int* count, const int* area, const long long* sum_y, const long long* sum_x, int max_points,
                          const unsigned char* window, int h, int w, int* out_py, int* out_px, int* out_info,
                          hipStream_t stream) {
  UNETDC_REQUIRE(count && area && sum_y && sum_x && out_py && out_px && out_info, "droplet_points: null pointer");
  UNETDC_REQUIRE(h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30) && max_points >= 1 &&
                     max_points <= RIPLEY_MAX_POINTS,
                 "droplet_points: bad geometry (sides 1..16384, max_points 1..2^20)");
  hipLaunchKernelGGL(spatial_points_kernel, dim3(1), dim3(256), 0, stream, count, area, sum_y, sum_x, max_points, window, h, w, out_py,
                     out_px, out_info);
  if (window)
    hipLaunchKernelGGL(spatial_window_count_kernel, dim3(grid_for((long)h * w, 256 * 16, 1024)), dim3(256), 0, stream, window, h * w,
                       out_info + 2);
  return check_launch("droplet points kernels");
}

// ---- the window's prefix counts -----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void spatial_window_rows_kernel(const unsigned char* __restrict__ window, int h, int w, RipleyPlanes p) {
  const int lane = threadIdx.x & 63;
  const int nb = (w + 63) >> 6;
  for (int y = blockIdx.x * 4 + (threadIdx.x >> 6); y < h; y += gridDim.x * 4) {         // uniform within a wave
    const unsigned char* row = window + (long)y * w;
    int run = 0;
    for (int b = 0; b < nb; ++b) {
      const int x = (b << 6) + lane;
      const unsigned long long m = __ballot(x < w && row[x] != 0);
      if (lane == 0) {
        p.bits[(long)y * nb + b] = m;
        p.blkpre[(long)y * nb + b] = run;
      }
      run += __popcll(m);
    }
    if (lane == 0) p.rowpre[y + 1] = run;                      // the row's own count; spatial_window_scan_kernel turns it into the prefix
  }
}

// rowpre[1 .. h] holds the rows' counts on entry, the inclusive prefix on exit; rowpre[0] = 0.  The exclusive scan of the counts
// written one place down is just that: rowpre[0 .. h) = the counts above a row, and the total goes to rowpre[h].
__global__ __launch_bounds__(256) void spatial_window_scan_kernel(int h, RipleyPlanes p) {
  __shared__ int s_w[4];
  const long long total = scan_plane<256>(p.rowpre + 1, p.rowpre, h, s_w);
  if (threadIdx.x == 0) p.rowpre[h] = (int)total;
}

// ---- the point sets -----------------------------------------------------------------------------------------------------------

// the largest r in 0..R with r * r < b2 (b2 >= 1)
__device__ __forceinline__ int ripley_border_radius(int b2, int R) {
  int r = (int)sqrtf((float)(b2 - 1));                         // proposes floor(sqrt(b2 - 1)); the comparisons decide
  while ((long long)r * r > (long long)b2 - 1) --r;
  while ((long long)(r + 1) * (r + 1) <= (long long)b2 - 1) ++r;
  return r < R ? r : R;
}

__global__ __launch_bounds__(256) void spatial_sets_kernel(const int* __restrict__ py, const int* __restrict__ px,
                                                          const int* __restrict__ n_points, int max_points, bool windowed, int h,
                                                          int w, int R, int n_sim, unsigned seed, RipleyPlanes p) {
  int N = *n_points;
  N = N < 0 ? 0 : N < max_points ? N : max_points;
  const int nb = (w + 63) >> 6;
  const int A = windowed ? p.rowpre[h] : h * w;
  const long total = (long)(A > 0 ? 1 + n_sim : 1) * N;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int set = (int)(idx / N), k = (int)(idx - (long)set * N);
    int y, x;
    if (set == 0) {
      y = py[k];
      x = px[k];
      y = y < 0 ? 0 : y < h ? y : h - 1;                       // the caller's points lie inside the image; nothing is read outside it
      x = x < 0 ? 0 : x < w ? x : w - 1;
    } else {
      const unsigned rowkey = aug_fmix32(aug_fmix32(seed) ^ ((unsigned)(set - 1) * RIPLEY_GOLDEN));
      const unsigned hi = aug_fmix32(rowkey ^ (2u * (unsigned)k)), lo = aug_fmix32(rowkey ^ (2u * (unsigned)k + 1u));
      const unsigned long long u = ((unsigned long long)hi << 32) | lo;
      int t = (int)__umul64hi(u, (unsigned long long)A);       // 0 .. A - 1
      if (!windowed) {
        y = t / w;
        x = t - y * w;
      } else {
        int lo_y = 0, hi_y = h - 1;                            // the largest y with rowpre[y] <= t
        while (lo_y < hi_y) {
          const int mid = (lo_y + hi_y + 1) >> 1;
          if (p.rowpre[mid] <= t) lo_y = mid; else hi_y = mid - 1;
        }
        y = lo_y;
        t -= p.rowpre[y];
        const int* pre = p.blkpre + (long)y * nb;
        int lo_b = 0, hi_b = nb - 1;                           // the largest block with blkpre <= t
        while (lo_b < hi_b) {
          const int mid = (lo_b + hi_b + 1) >> 1;
          if (pre[mid] <= t) lo_b = mid; else hi_b = mid - 1;
        }
        t -= pre[lo_b];
        unsigned long long m = p.bits[(long)y * nb + lo_b];
        for (int q = 0; q < t && m; ++q) m &= m - 1;           // drop the t lowest set bits (t < 64)
        x = (lo_b << 6) + (m ? __ffsll((long long)m) - 1 : 0);
        x = x < w ? x : w - 1;
      }
    }
    int m = y + 1 < x + 1 ? y + 1 : x + 1;
    m = m < h - y ? m : h - y;
    m = m < w - x ? m : w - x;
    int b2 = m * m;                                            // m <= 8192
    if (windowed) {
      const int d = p.d2[(long)y * w + x];
      b2 = d < b2 ? d : b2;
    }
    const long at = (long)set * max_points + k;
    p.pts[at] = ((unsigned)y << 16) | (unsigned)x;
    p.e[at] = b2 >= 1 ? ripley_border_radius(b2, R) : 0;      // b2 = 0: a given point outside the window, which has no margin
  }
}

__global__ __launch_bounds__(256) void spatial_eligible_kernel(const int* __restrict__ n_points, int max_points, int R,
                                                              const int* __restrict__ window_a, RipleyPlanes p,
                                                              int* __restrict__ out_n,
                                                              unsigned long long* __restrict__ out_pairs,
                                                              unsigned long long* __restrict__ out_pairs_all) {
  extern __shared__ int hist[];                                // [R + 1]
  int N = *n_points;
  N = N < 0 ? 0 : N < max_points ? N : max_points;
  const int set = blockIdx.x;
  if (set > 0 && window_a && *window_a == 0) N = 0;            // no pixel to draw from: the simulation rows are zero
  for (int r = threadIdx.x; r <= R; r += 256) hist[r] = 0;
  __syncthreads();
  const int* e = p.e + (long)set * max_points;
  for (int k = threadIdx.x; k < N; k += 256) atomicAdd(&hist[e[k]], 1);
  __syncthreads();
  for (int r = threadIdx.x; r <= R; r += 256) {
    int s = 0;
    for (int q = r; q <= R; ++q) s += hist[q];
    const long at = (long)set * (R + 1) + r;
    out_n[at] = s;
    out_pairs[at] = 0;
    out_pairs_all[at] = 0;
  }
}

// the smallest c >= 0 with c * c >= d2, for d2 <= 65536 (exact in float; the comparisons decide all the same)
__device__ __forceinline__ int ripley_pair_radius(int d2) {
  int c = (int)sqrtf((float)d2);
  while (c * c < d2) ++c;
  while (c > 0 && (c - 1) * (c - 1) >= d2) --c;
  return c;
}

__global__ __launch_bounds__(256) void spatial_pairs_kernel(const int* __restrict__ n_points, int max_points, int R,
                                                           const int* __restrict__ window_a, RipleyPlanes p,
                                                           unsigned long long* __restrict__ out_pairs,
                                                           unsigned long long* __restrict__ out_pairs_all) {
  extern __shared__ unsigned long long lds[];
  unsigned long long* acc = lds;                               // [2][R + 1] the workgroup's sums
  unsigned* tile = reinterpret_cast<unsigned*>(lds + 2 * (R + 1));       // [RIPLEY_TILE]
  int* hist = reinterpret_cast<int*>(tile + RIPLEY_TILE) + (threadIdx.x >> 6) * (R + 1);   // [4][R + 1], this wave's
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int set = blockIdx.y;
  int N = *n_points;
  N = N < 0 ? 0 : N < max_points ? N : max_points;
  if (set > 0 && window_a && *window_a == 0) N = 0;            // no pixel to draw from: the simulation rows stay zero
  const unsigned* pts = p.pts + (long)set * max_points;
  const int* e = p.e + (long)set * max_points;
  const int R2 = R * R;
  for (int r = threadIdx.x; r < 2 * (R + 1); r += 256) acc[r] = 0;
  for (int r = lane; r <= R; r += 64) hist[r] = 0;
  unsigned long long sum_pairs[RIPLEY_CHUNKS], sum_all[RIPLEY_CHUNKS];
#pragma unroll
  for (int q = 0; q < RIPLEY_CHUNKS; ++q) sum_pairs[q] = sum_all[q] = 0;
  for (int i0 = blockIdx.x * 4; i0 < N; i0 += gridDim.x * 4) {           // uniform over the workgroup: every wave meets every barrier
    const int i = i0 + wave;
    const bool active = i < N;
    const unsigned pi = active ? pts[i] : 0u;
    const int yi = (int)(pi >> 16), xi = (int)(pi & 0xffffu), ei = active ? e[i] : -1;
    for (int t0 = 0; t0 < N; t0 += RIPLEY_TILE) {
      const int tn = N - t0 < RIPLEY_TILE ? N - t0 : RIPLEY_TILE;
      __syncthreads();                                         // the tile's readers are done; the zeroed bins are in place
      for (int j = threadIdx.x; j < tn; j += 256) tile[j] = pts[t0 + j];
      __syncthreads();
      if (active) {
        for (int j = lane; j < tn; j += 64) {
          const unsigned pj = tile[j];
          const int dy = (int)(pj >> 16) - yi, dx = (int)(pj & 0xffffu) - xi;
          const int d2 = dy * dy + dx * dx;                    // < 2^29
          if (d2 <= R2 && t0 + j != i) atomicAdd(&hist[ripley_pair_radius(d2)], 1);
        }
      }
    }
    __syncthreads();                                           // this wave's bins are complete
    int carry = 0;
#pragma unroll
    for (int q = 0; q < RIPLEY_CHUNKS; ++q) {
      const int r = (q << 6) + lane;
      if ((q << 6) > R) break;                                 // uniform
      int v = r <= R ? hist[r] : 0;
      if (r <= R) hist[r] = 0;                                 // for the wave's next i
      v = wave_incl_scan(v, lane) + carry;
      carry = __shfl(v, 63, 64);
      sum_all[q] += (unsigned)v;
      if (r <= ei) sum_pairs[q] += (unsigned)v;
    }
  }
  __syncthreads();                                             // acc is zeroed (and with N = 0 nothing else happened)
#pragma unroll
  for (int q = 0; q < RIPLEY_CHUNKS; ++q) {
    const int r = (q << 6) + lane;
    if (r <= R) {
      if (sum_pairs[q]) atomicAdd(&acc[r], sum_pairs[q]);
      if (sum_all[q]) atomicAdd(&acc[R + 1 + r], sum_all[q]);
    }
  }
  __syncthreads();
  for (int r = threadIdx.x; r <= R; r += 256) {
    const long at = (long)set * (R + 1) + r;
    if (acc[r]) atomicAdd(out_pairs + at, acc[r]);
    if (acc[R + 1 + r]) atomicAdd(out_pairs_all + at, acc[R + 1 + r]);
  }
}

int launch_ripley_counts(const int* py, const int* px, const int* n_points, int max_points, const unsigned char* window, int h,
                         int w, int rmax, int n_sim, unsigned seed, void* workspace, long workspace_bytes, int* out_n,
                         long long* out_pairs, long long* out_pairs_all, hipStream_t stream) {
  UNETDC_REQUIRE(py && px && n_points && workspace && out_n && out_pairs && out_pairs_all, "ripley_counts: null pointer");
  const auto lay = ripley_layout(h, w, max_points, rmax, n_sim, workspace);
  UNETDC_REQUIRE(lay.ok, "ripley_counts: bad geometry (sides 1..16384, rmax 1..256, n_sim 0..999, max_points 1..2^20)");
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ripley_counts: workspace must be 8-byte aligned");
  if (int rc = require_workspace("ripley_counts", workspace_bytes, lay.bytes)) return rc;
  const RipleyPlanes& p = lay.planes;
  const int sets = 1 + n_sim;
  if (window) {
    if (int rc = launch_edt_sq(window, h, w, p.d2, p.g, p.g_bytes, stream)) return rc;
    hipLaunchKernelGGL(spatial_window_rows_kernel, dim3(grid_for(h, 4, 4096)), dim3(256), 0, stream, window, h, w, p);
    hipLaunchKernelGGL(spatial_window_scan_kernel, dim3(1), dim3(256), 0, stream, h, p);
  }
  hipLaunchKernelGGL(spatial_sets_kernel, dim3(grid_for((long)sets * max_points, 256, 4096)), dim3(256), 0, stream, py, px, n_points,
                     max_points, window != nullptr, h, w, rmax, n_sim, seed, p);
  auto* pairs = reinterpret_cast<unsigned long long*>(out_pairs);
  auto* pairs_all = reinterpret_cast<unsigned long long*>(out_pairs_all);
  const int* window_a = window ? p.rowpre + h : nullptr;
  hipLaunchKernelGGL(spatial_eligible_kernel, dim3(sets), dim3(256), (size_t)(rmax + 1) * 4, stream, n_points, max_points, rmax,
                     window_a, p, out_n, pairs, pairs_all);
  const int gx = grid_for(max_points, 4, std::max(1, 4096 / sets));
  const size_t lds = (size_t)2 * (rmax + 1) * 8 + (size_t)RIPLEY_TILE * 4 + (size_t)4 * (rmax + 1) * 4;
  hipLaunchKernelGGL(spatial_pairs_kernel, dim3(gx, sets), dim3(256), lds, stream, n_points, max_points, rmax, window_a, p, pairs,
                     pairs_all);
  return check_launch("ripley kernels");
}

}  // namespace unetdc
