// Difference map of a predicted mask against an annotated one: the class plane
//   c = (pred != 0) | (gt != 0) << 1        0 black (TN), 1 green (FP), 2 red (FN), 3 yellow (TP)
// painted in the reference's colours (train_DC_focal.py:create_difference_map / overlay_difference), and its 8-CONNECTED
// regions of equal class (count_color_regions_in_memory), black included, with one table row per coloured region.
//
//   diff_init_kernel    cls[i] = c, L[i] = the head of i's run of equal class within 64 consecutive pixels of its row (a ballot:
//                       no atomic), the accumulators 0; its first threads clear the twelve image integers
//   diff_merge_kernel   union-find of ccl_uf.h over ALL pixels: of the W, NW, N, NE neighbours of equal class a pixel unites
//                       with those that the runs and the other unions do not already imply (in a flat region: one per run)
//   diff_stats_kernel   at the root: area, sums of rows and columns, and the OR of the classes among the 8 neighbours.  The
//                       lanes of a wave that share a root send ONE add per quantity (for_each_wave_key, wave_ops.h: the black class is one
//                       region of about a million pixels on a micrograph, whose pixels would all land on the same three words);
//                       pixels[] takes one add per wave and class
//   diff_count_kernel   regions[] and kept[] at the root pixels, and per 1024 pixels the number of table rows
//   (ccl.hip's scan)    exclusive scan of those numbers; the total is *out_count
//   diff_emit_kernel    the rows (class 1..3, area >= min_area) in increasing root order = raster order of the first pixel
//   diff_paint_kernel   the two pictures: a lane takes 4 consecutive pixels, 12 bytes per plane = three whole dwords
//
// Byte and integer work only.  Every kernel is a grid-stride loop whose trip count is uniform within a wave where it ballots
// or shuffles.  Integer atomics and the shared union-find: the outputs depend on no order.
#include "kernels.h"
#include "ccl_uf.h"
#include "wave_ops.h"

namespace unetdc {

constexpr int DIFF_THREADS = 256;
constexpr int DIFF_GRID_CAP = 4096;               // workgroups of the per-pixel kernels: 1 048 576 pixels a trip
constexpr int DIFF_STATS_GRID_CAP = 1024;         // of the stats kernel: 262 144 pixels a trip, so that a wave makes several
constexpr int DIFF_BLK = 1024;                    // pixels per scan block
constexpr int DIFF_BLOCK_GRID_CAP = 1024;         // workgroups of the count and emit kernels: 1 048 576 pixels a trip
constexpr int DIFF_MAX_SIDE = 16384;

struct DiffPlanes {
  unsigned long long *sy, *sx;
  int *L, *area, *nbr, *blocksum;
  unsigned char* cls;
};

// A SEGMENT is 64 consecutive pixels of the flat image from a multiple of 64: the lanes of one wave here (256 threads, bases
// that are multiples of 256).  L[i] = the first pixel of i's run of equal class within its segment and its row: a forest
// before the first atomic, in which a run of 64 black pixels is already one class.
__global__ __launch_bounds__(DIFF_THREADS) void diff_init_kernel(const unsigned char* __restrict__ pred,
                                                                 const unsigned char* __restrict__ gt, DiffPlanes p, int n, int w,
                                                                 long long* __restrict__ out_image) {
  if (blockIdx.x == 0 && threadIdx.x < 12) out_image[threadIdx.x] = 0;
  const int lane = threadIdx.x & 63;
  for (int base = blockIdx.x * DIFF_THREADS; base < n; base += gridDim.x * DIFF_THREADS) {   // uniform in the wave
    const int i = base + threadIdx.x;
    const bool live = i < n;
    const int c = live ? (pred[i] != 0 ? 1 : 0) | (gt[i] != 0 ? 2 : 0) : 0;
    const int left = __shfl_up(c, 1, 64);
    const unsigned long long heads = __ballot(live && (lane == 0 || i % w == 0 || left != c));
    if (!live) continue;                                    // the live lanes are a prefix of the wave, lane 0 a head
    const unsigned long long upto = heads & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);
    p.cls[i] = (unsigned char)c;
    p.L[i] = i - (lane - (63 - __clzll((long long)upto)));
    p.area[i] = 0;
    p.nbr[i] = 0;
    p.sy[i] = 0ull;
    p.sx[i] = 0ull;
  }
}

// The unions that the runs of diff_init_kernel leave open.  W: only across a segment seam.  N: only where W or NW differs --
// else W is of the class, W's own N edge (or what implies it, by induction along the row) joins W to NW, and NW is joined to N
// as a horizontal pair.  NW and NE: only where N differs (N is joined to both as horizontal pairs), NW also only where W
// differs (W is joined to NW as a vertical pair).  Inside a flat region that leaves one union per segment and row.
__global__ void diff_merge_kernel(const unsigned char* __restrict__ cls, int* __restrict__ L, int h, int w) {
  const int n = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int y = i / w, x = i - y * w;
    const unsigned char c = cls[i];
    const bool west = x > 0 && cls[i - 1] == c;
    if (west && (i & 63) == 0) ccl_unite(L, i, i - 1);
    if (y == 0) continue;
    const bool nw = x > 0 && cls[i - w - 1] == c;
    if (cls[i - w] == c) {
      if (!(west && nw)) ccl_unite(L, i, i - w);
      continue;
    }
    if (nw && !west) ccl_unite(L, i, i - w - 1);
    if (x + 1 < w && cls[i - w + 1] == c) ccl_unite(L, i, i - w + 1);
  }
}

// bit k: some 8-neighbour of (y, x) inside the image has class k != c
__device__ __forceinline__ int diff_neighbor_mask(const unsigned char* __restrict__ cls, int i, int y, int x, int h, int w, int c) {
  int m = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const int yy = y + dy, xx = x + dx;
      if (yy >= 0 && yy < h && xx >= 0 && xx < w) m |= 1 << cls[i + dy * w + dx];
    }
  }
  return m & ~(1 << c);
}

// what a wave has gathered for one root and not sent yet; every field is uniform in the wave
struct DiffPending {
  int root, count, mask;
  long long sy, sx;
};

__device__ __forceinline__ void diff_flush(const DiffPlanes& p, const DiffPending& q, int lane) {
  if (lane != 0 || q.root < 0) return;
  atomicAdd(&p.area[q.root], q.count);
  atomicAdd(&p.sy[q.root], (unsigned long long)q.sy);
  atomicAdd(&p.sx[q.root], (unsigned long long)q.sx);
  if (q.mask) atomicOr(&p.nbr[q.root], q.mask);
}

__global__ __launch_bounds__(DIFF_THREADS) void diff_stats_kernel(DiffPlanes p, int h, int w, long long* __restrict__ out_image) {
  const int n = h * w, lane = threadIdx.x & 63;
  int px0 = 0, px1 = 0, px2 = 0, px3 = 0;
  DiffPending held = {-1, 0, 0, 0ll, 0ll};
  for (int base = blockIdx.x * DIFF_THREADS; base < n; base += gridDim.x * DIFF_THREADS) {
    const int i = base + threadIdx.x;
    const bool live = i < n;
    int r = -1, y = 0, x = 0, m = 0;
    if (live) {
      r = ccl_find(p.L, i);
      p.L[i] = r;                                           // a root keeps L[r] = r
      y = i / w;
      x = i - y * w;
      const int c = p.cls[i];
      m = diff_neighbor_mask(p.cls, i, y, x, h, w, c);
      px0 += c == 0;
      px1 += c == 1;
      px2 += c == 2;
      px3 += c == 3;
    }
    for_each_wave_key(r, live, [&](int lead, int r0, unsigned long long same) {
      const bool mine = live && r == r0;
      const int cnt = __popcll(same);
      int ys, xs, ms;
      if (cnt > 1) {                                        // uniform
        ys = wave_sum(mine ? y : 0);                        // at most 64 * 16383
        xs = wave_sum(mine ? x : 0);
        ms = wave_or(mine ? m : 0);
      } else {                                              // the only lane of its root: no reduction
        ys = __shfl(y, lead, 64);
        xs = __shfl(x, lead, 64);
        ms = __shfl(m, lead, 64);
      }
      // The root of the wave's last run is kept over the trips of the loop: a wave that walks a flat region sends one set of
      // adds for all of its trips, not one per trip (every wave of a black image would otherwise queue on the same words).
      if (r0 != held.root) {
        diff_flush(p, held, lane);
        held = {r0, 0, 0, 0ll, 0ll};
      }
      held.count += cnt;
      held.sy += ys;
      held.sx += xs;
      held.mask |= ms;
    });
  }
  diff_flush(p, held, lane);
  const int px[4] = {wave_sum(px0), wave_sum(px1), wave_sum(px2), wave_sum(px3)};
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (px[c]) atomic_add64(out_image + c, px[c]);
  }
}

// pixel i is the root of a table row
__device__ __forceinline__ bool diff_row(const DiffPlanes& p, int i, int min_area) {
  return p.cls[i] != 0 && p.L[i] == i && p.area[i] >= min_area;
}

// blocksum[b] = table rows among the pixels of block b; out_image[4..7] += regions, [8..11] += regions of at least min_area
__global__ __launch_bounds__(DIFF_THREADS) void diff_count_kernel(DiffPlanes p, int n, int nblocks, int min_area,
                                                                  long long* __restrict__ out_image) {
  __shared__ int red[4];
  int reg0 = 0, reg1 = 0, reg2 = 0, reg3 = 0, kept0 = 0, kept1 = 0, kept2 = 0, kept3 = 0;
  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {   // uniform in the workgroup
    int rows = 0;
    for (int k = threadIdx.x; k < DIFF_BLK; k += DIFF_THREADS) {
      const int i = b * DIFF_BLK + k;
      if (i >= n || p.L[i] != i) continue;
      const int c = p.cls[i];
      const bool big = p.area[i] >= min_area;
      reg0 += c == 0;
      reg1 += c == 1;
      reg2 += c == 2;
      reg3 += c == 3;
      kept0 += big && c == 0;
      kept1 += big && c == 1;
      kept2 += big && c == 2;
      kept3 += big && c == 3;
      rows += big && c != 0;
    }
    rows = block_sum<DIFF_THREADS>(rows, red);
    if (threadIdx.x == 0) p.blocksum[b] = rows;
    __syncthreads();                                        // red[] is written again on the next trip
  }
  const int sums[8] = {wave_sum(reg0),  wave_sum(reg1),  wave_sum(reg2),  wave_sum(reg3),
                       wave_sum(kept0), wave_sum(kept1), wave_sum(kept2), wave_sum(kept3)};
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (sums[q]) atomic_add64(out_image + 4 + q, sums[q]);
  }
}

// a thread takes 4 consecutive pixels of its block; an exclusive scan of the 256 counts gives every row its rank
__global__ __launch_bounds__(DIFF_THREADS) void diff_emit_kernel(DiffPlanes p, int n, int nblocks, int min_area, int max_out,
                                                                 int* __restrict__ out_class, int* __restrict__ out_area,
                                                                 long long* __restrict__ out_sy, long long* __restrict__ out_sx,
                                                                 int* __restrict__ out_nbr) {
  __shared__ int s_w[DIFF_THREADS / 64];
  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {   // uniform in the workgroup
    const int base = b * DIFF_BLK + threadIdx.x * 4;
    bool k[4];
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k[j] = base + j < n && diff_row(p, base + j, min_area);
      c += k[j] ? 1 : 0;
    }
    int rank = p.blocksum[b] + block_excl_scan<DIFF_THREADS>(c, s_w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!k[j]) continue;
      const int i = base + j;
      if (rank < max_out) {
        out_class[rank] = p.cls[i];
        out_area[rank] = p.area[i];
        out_sy[rank] = (long long)p.sy[i];
        out_sx[rank] = (long long)p.sx[i];
        out_nbr[rank] = p.nbr[i];
      }
      ++rank;
    }
  }
}

// Group g = pixels 4 g .. 4 g + 3 of the flat image.  WIDE (every given plane 4-byte aligned): a whole group reads pred and
// gt as one dword each, rgb as three, and writes three dwords per output; the last group of an image whose pixel count is no
// multiple of 4, and every group without WIDE, goes byte by byte.
template <bool WIDE>
__global__ void diff_paint_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                  const unsigned char* __restrict__ rgb, int n, unsigned char* __restrict__ out_diff,
                                  unsigned char* __restrict__ out_overlay) {
  const int groups = (n + 3) / 4;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
    const int i0 = 4 * g;
    if (WIDE && i0 + 4 <= n) {
      const unsigned int pw = *reinterpret_cast<const unsigned int*>(pred + i0);
      const unsigned int gw = *reinterpret_cast<const unsigned int*>(gt + i0);
      unsigned int col[3] = {0u, 0u, 0u}, set[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool a = ((pw >> (8 * k)) & 0xffu) != 0, b = ((gw >> (8 * k)) & 0xffu) != 0;
        const unsigned int ch[3] = {b ? 255u : 0u, a ? 255u : 0u, 0u};            // red with the annotation, green with the prediction
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int byte = 3 * k + q;
          col[byte >> 2] |= ch[q] << (8 * (byte & 3));
          if (a || b) set[byte >> 2] |= 0xffu << (8 * (byte & 3));
        }
      }
      const long o = 3l * i0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (out_diff) reinterpret_cast<unsigned int*>(out_diff + o)[q] = col[q];
        if (out_overlay) {
          const unsigned int v = reinterpret_cast<const unsigned int*>(rgb + o)[q];
          reinterpret_cast<unsigned int*>(out_overlay + o)[q] = (v & ~set[q]) | col[q];
        }
      }
      continue;
    }
    for (int i = i0; i < min(i0 + 4, n); ++i) {
      const bool a = pred[i] != 0, b = gt[i] != 0;
      const unsigned char ch[3] = {(unsigned char)(b ? 255 : 0), (unsigned char)(a ? 255 : 0), 0};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (out_diff) out_diff[3l * i + q] = ch[q];
        if (out_overlay) out_overlay[3l * i + q] = (a || b) ? ch[q] : rgb[3l * i + q];
      }
    }
  }
}

static bool diff_geometry(int h, int w) {
  return h >= 1 && w >= 1 && h <= DIFF_MAX_SIDE && w <= DIFF_MAX_SIDE && (long)h * w < (1L << 30);
}

// the two coordinate sums (8 bytes each), the union-find, the areas and the neighbour masks (4 each), one block sum per 1024
// pixels and 16 more, the class bytes, 64 spare bytes: 29 n + 4 ceil(n / 1024) + 128
static Layout<DiffPlanes> diff_layout(int h, int w, void* workspace) {
  if (!diff_geometry(h, w)) return {false, 0, {}};
  const long n = (long)h * w, nb = (n + DIFF_BLK - 1) / DIFF_BLK;
  Carver c(workspace);
  DiffPlanes p;
  p.sy = c.take<unsigned long long>(n);
  p.sx = c.take<unsigned long long>(n);
  p.L = c.take<int>(n);
  p.area = c.take<int>(n);
  p.nbr = c.take<int>(n);
  p.blocksum = c.take<int>(nb + 16);
  p.cls = c.take<unsigned char>(n);
  c.slack(64);
  return {true, c.bytes(), p};
}
long diff_regions_workspace_bytes(int h, int w) { return diff_layout(h, w, nullptr).bytes; }

static bool diff_aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }

int launch_diff_regions(const unsigned char* pred, const unsigned char* gt, int h, int w, int min_area, void* workspace,
                        long workspace_bytes, long long* out_image, int* out_count, int* out_class, int* out_area,
                        long long* out_sumy, long long* out_sumx, int* out_neighbors, int max_out, hipStream_t stream) {
  UNETDC_REQUIRE(pred && gt && workspace && out_image && out_count, "diff_regions: null pointer");
  const auto lay = diff_layout(h, w, workspace);
  UNETDC_REQUIRE(lay.ok && min_area >= 1 && max_out >= 0,
                 "diff_regions: bad geometry (sides 1..16384, h * w < 2^30, min_area >= 1, max_out >= 0)");
  UNETDC_REQUIRE(max_out == 0 || (out_class && out_area && out_sumy && out_sumx && out_neighbors),
                 "diff_regions: null table with max_out > 0");
  if (int rc = require_workspace("diff_regions", workspace_bytes, lay.bytes)) return rc;
  UNETDC_REQUIRE(diff_aligned(workspace, 8) && diff_aligned(out_image, 8) && diff_aligned(out_sumy, 8) &&
                     diff_aligned(out_sumx, 8) && diff_aligned(out_count, 4) && diff_aligned(out_class, 4) &&
                     diff_aligned(out_area, 4) && diff_aligned(out_neighbors, 4),
                 "diff_regions: workspace, out_image and the sums must be 8-byte aligned, the int32 outputs 4-byte aligned");
  const DiffPlanes& p = lay.planes;
  const int n = h * w, nb = (n + DIFF_BLK - 1) / DIFF_BLK;
  const dim3 grid(grid_for(n, DIFF_THREADS, DIFF_GRID_CAP)), bgrid(grid_for(nb, 1, DIFF_BLOCK_GRID_CAP)), block(DIFF_THREADS);
  hipLaunchKernelGGL(diff_init_kernel, grid, block, 0, stream, pred, gt, p, n, w, out_image);
  hipLaunchKernelGGL(diff_merge_kernel, grid, block, 0, stream, p.cls, p.L, h, w);
  hipLaunchKernelGGL(diff_stats_kernel, dim3(grid_for(n, DIFF_THREADS, DIFF_STATS_GRID_CAP)), block, 0, stream, p, h, w, out_image);
  hipLaunchKernelGGL(diff_count_kernel, bgrid, block, 0, stream, p, n, nb, min_area, out_image);
  launch_ccl_scan(p.blocksum, nb, out_count, stream);
  hipLaunchKernelGGL(diff_emit_kernel, bgrid, block, 0, stream, p, n, nb, min_area, max_out, out_class, out_area, out_sumy,
                     out_sumx, out_neighbors);
  return check_launch("diff region kernels");
}

int launch_diff_paint(const unsigned char* pred, const unsigned char* gt, const unsigned char* rgb, int h, int w,
                      unsigned char* out_diff, unsigned char* out_overlay, hipStream_t stream) {
  UNETDC_REQUIRE(pred && gt, "diff_paint: null pointer");
  UNETDC_REQUIRE(diff_geometry(h, w), "diff_paint: bad geometry (sides 1..16384, h * w < 2^30)");
  UNETDC_REQUIRE(out_diff || out_overlay, "diff_paint: no output given");
  UNETDC_REQUIRE(!out_overlay || rgb, "diff_paint: out_overlay needs rgb");
  const int n = h * w;
  const bool wide = diff_aligned(pred, 4) && diff_aligned(gt, 4) && diff_aligned(out_diff, 4) && diff_aligned(out_overlay, 4) &&
                    (!out_overlay || diff_aligned(rgb, 4));
  const dim3 grid(grid_for((n + 3) / 4, DIFF_THREADS, DIFF_GRID_CAP)), block(DIFF_THREADS);
  if (wide)
    hipLaunchKernelGGL(diff_paint_kernel<true>, grid, block, 0, stream, pred, gt, rgb, n, out_diff, out_overlay);
  else
    hipLaunchKernelGGL(diff_paint_kernel<false>, grid, block, 0, stream, pred, gt, rgb, n, out_diff, out_overlay);
  return check_launch("diff_paint_kernel");
}

}  // namespace unetdc
