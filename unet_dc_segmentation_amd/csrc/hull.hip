// Convex hull of every droplet of an int32 label map, and from it the integers of solidity and the Feret diameters
// (the rule is stated once in utils/droplet_hull.py).  The point set of a label is the union of the closed
// unit squares of its pixels, so every hull vertex is a lattice point and every quantity an exact integer.  Per corner level
// t = min_y .. max_y + 1 of a label only the leftmost and the rightmost pixel corner can be a vertex: the leftmost pixel of the
// rows t - 1 and t, and one past the rightmost.  The left chain of the hull is the lower convex hull of the left candidates
// read as (t, x), the right chain the upper hull of the right ones; the two never share a point.
//
//   hull_init_kernel      min_y INT_MAX, max_y -1 per label; out zeros
//   hull_extent_kernel    the frame of label_props_kernel (shape.hip): one wave per 64 consecutive pixels of a row, runs of
//                         equal labels (row_unit and wave_runs, wave_ops.h); one atomicMin / atomicMax of y per run
//   hull_scan_kernel      one workgroup: exclusive scan of (height + 1) over the labels into segment offsets (a label of
//                         height H has H + 1 corner levels), in coalesced tiles of 4096 labels; the sum of the heights decides
//                         *out_rows and the overflow flag
//   hull_fill_kernel      the used part of the two candidate planes: INT_MAX left, -1 right (what an empty level keeps)
//   hull_rows_kernel      the same frame: a run x0 .. x1 of row y gives atomicMin(x0) to the left candidates of levels y and
//                         y + 1 and atomicMax(x1 + 1) to the right ones
//   hull_chain_kernel     one wave per (label, side).  The levels are cut into 64 chunks, lane l runs Andrew's monotone chain over
//                         its chunk in place (the stack never outruns the read cursor), then lane 0 runs the same chain over the
//                         concatenation of the 64 results, again in place: it is still sorted by y, and the hull of hulls is
//                         the hull.  A pass runs in LDS (a dependent load there costs a tenth of one from memory) when it fits:
//                         the first with at most 2048 levels, the second with at most 2048 points in the 64 results.  A label of at most 64 levels has one level
//                         per lane, kept in a register, and the second pass is the whole chain.  Integer cross products;
//                         collinear points are dropped.  Vertices are kept as y << 15 | x.
//   hull_caliper_kernel   one wave per label over the polygon left chain down, right chain up: the shoelace sum, the largest
//                         squared vertex distance over all pairs, and per edge the largest cross product with a vertex; the
//                         wave reduces with integer max, and with the minimum of Wc^2 / Wl compared in 128 bits.
// Integer atomic min / max and sequential chains only: the result does not depend on the order in which anything runs.
#include "kernels.h"
#include "wave_ops.h"
#include "workspace.h"

namespace unetdc {

enum { H_H2 = 0, H_F2, H_WC, H_WL, H_NV };
static_assert(H_NV + 1 == HULL_QUANTITIES, "hull quantities");

constexpr int HULL_LEFT_EMPTY = 0x7fffffff, HULL_RIGHT_EMPTY = -1;
constexpr int HULL_MAX_GROUPS = 4096;
constexpr int HULL_MAX_CHAINS = 1 << 15;     // one-wave workgroups of hull_chain_kernel: one per (label, side) up to 16384 labels
constexpr int HULL_LDS_POINTS = 2048;        // levels, and chunk vertices, of one side of one label that a chain pass holds in LDS (8 KB each)

struct HullPlanes {
  int* ctl;        // [0] overflow flag, [1] used slots of the candidate planes
  int *min_y, *max_y;   // [max_out]
  int* off;        // [max_out] first slot of a label's segment
  int* count;      // [2 * max_out] vertices of the left and of the right chain
  int *left, *right;    // [slots] candidates, then the chains
  long slots;
};

static Layout<HullPlanes> hull_layout(int h, int w, int max_out, int max_rows, void* workspace) {
  if (!(h > 0 && w > 0 && h <= 16384 && w <= 16384 && max_out >= 0 && max_rows >= 0 && max_rows <= (1 << 28))) return {false, 0, {}};
  Carver c(workspace);
  HullPlanes p;
  // a label with pixels takes (height + 1) slots and there are at most h * w of those: max_rows heights and one more each
  p.slots = (long)max_rows + std::min((long)max_out, (long)h * w);
  p.ctl = c.take<int>(16);
  p.min_y = c.take<int>(max_out, 64);
  p.max_y = c.take<int>(max_out, 64);
  p.off = c.take<int>(max_out, 64);
  p.count = c.take<int>(2L * max_out, 64);
  p.left = c.take<int>(p.slots, 64);
  p.right = c.take<int>(p.slots, 64);
  return {true, c.bytes(), p};
}
long label_hull_workspace_bytes(int h, int w, int max_out, int max_rows) { return hull_layout(h, w, max_out, max_rows, nullptr).bytes; }

__global__ void hull_init_kernel(HullPlanes p, int max_out, long long* __restrict__ out) {
  const long n = (long)HULL_QUANTITIES * max_out;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    out[i] = 0ll;
    if (i < max_out) p.min_y[i] = HULL_LEFT_EMPTY, p.max_y[i] = -1;
  }
}

// What a wave knows about its 64 pixels of row y: the label of this lane (0 outside 1..max_out), whether the lane heads a run
// of a label, and the run's last column.
struct HullRun {
  int k, y, x0, x1;
  bool head;
};
__device__ __forceinline__ bool hull_run(const int* __restrict__ label, int max_out, int w, int chunks, long u, HullRun& r) {
  const int lane = threadIdx.x & 63;
  const RowUnit px = row_unit(u, chunks, w, lane);
  int k = px.in ? label[px.i] : 0;
  if (k < 0 || k > max_out) k = 0;                          // labels past the capacity are skipped, never written
  if (__ballot(k > 0) == 0ull) return false;                // wave-uniform: nothing but background here
  const WaveRuns runs = wave_runs(k, lane);
  r.k = k, r.y = px.y, r.x0 = px.x, r.x1 = px.x + runs.len - 1;
  r.head = k > 0 && runs.head;
  return true;
}

__global__ __launch_bounds__(256) void hull_extent_kernel(const int* __restrict__ label, int max_out, int h, int w, HullPlanes p) {
  const int chunks = (w + 63) >> 6;
  const long units = (long)h * chunks, stride = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += stride) {   // uniform within a wave
    HullRun r;
    if (!hull_run(label, max_out, w, chunks, u, r)) continue;
    if (r.head) {
      atomicMin(p.min_y + r.k - 1, r.y);
      atomicMax(p.max_y + r.k - 1, r.y);
    }
  }
}

// One workgroup of 1024 walks the labels in tiles of 4096, four consecutive labels per thread: an inclusive scan of the slots
// inside each wave (shuffles), the 16 wave totals through LDS, the running totals in registers (uniform).  Offsets are written as
// they come; nothing reads them when the rows overflow.  The running sums are 64-bit.
__global__ __launch_bounds__(1024) void hull_scan_kernel(HullPlanes p, int max_out, int max_rows, int* __restrict__ out_rows) {
  __shared__ int s_rows[16], s_slots[16];                   // a tile's sums stay below 4096 * 16385 < 2^26
  const int* __restrict__ min_y = p.min_y;
  const int* __restrict__ max_y = p.max_y;
  int* __restrict__ off = p.off;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  long long run_rows = 0, run_slots = 0;
  for (long base = 0; base < max_out; base += 4096) {
    const long k0 = base + 4 * t;
    int slots[4], mine = 0, rows = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int top = k0 + j < max_out ? max_y[k0 + j] : -1;
      const int height = top >= 0 ? top - min_y[k0 + j] + 1 : 0;
      slots[j] = height ? height + 1 : 0;
      mine += slots[j];
      rows += height;
    }
    const int incl = wave_incl_scan(mine, lane);
    rows = wave_sum(rows);
    if (lane == 63) s_slots[wave] = incl, s_rows[wave] = rows;
    __syncthreads();
    int before = 0, tile_slots = 0, tile_rows = 0;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int q = s_slots[v];
      before += v < wave ? q : 0;
      tile_slots += q;
      tile_rows += s_rows[v];
    }
    long long at = run_slots + before + incl - mine;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k0 + j < max_out) off[k0 + j] = (int)at;
      at += slots[j];
    }
    run_slots += tile_slots;
    run_rows += tile_rows;
    __syncthreads();
  }
  if (t == 0) {
    const bool over = run_rows > max_rows;
    *out_rows = over ? max_rows + 1 : (int)run_rows;
    p.ctl[0] = over;
    p.ctl[1] = over ? 0 : (int)run_slots;
  }
}

__global__ void hull_fill_kernel(HullPlanes p) {
  const int n = p.ctl[1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    p.left[i] = HULL_LEFT_EMPTY, p.right[i] = HULL_RIGHT_EMPTY;
}

__global__ __launch_bounds__(256) void hull_rows_kernel(const int* __restrict__ label, int max_out, int h, int w, HullPlanes p) {
  if (p.ctl[0]) return;                                     // more rows than the planes hold
  const int chunks = (w + 63) >> 6;
  const long units = (long)h * chunks, stride = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += stride) {   // uniform within a wave
    HullRun r;
    if (!hull_run(label, max_out, w, chunks, u, r)) continue;
    if (r.head) {
      const int o = p.off[r.k - 1] + (r.y - p.min_y[r.k - 1]);      // level y; level y + 1 is the label's as well
      atomicMin(p.left + o, r.x0);
      atomicMin(p.left + o + 1, r.x0);
      atomicMax(p.right + o, r.x1 + 1);
      atomicMax(p.right + o + 1, r.x1 + 1);
    }
  }
}

__device__ __forceinline__ int hull_pack(int x, int y) { return (y << 15) | x; }     // 0 <= x, y <= 16384
__device__ __forceinline__ int hull_x(int v) { return v & 32767; }
__device__ __forceinline__ int hull_y(int v) { return v >> 15; }

// Push the packed point v on the chain seg[0 .. n): pop while the last two points and v do not turn strictly the way of the
// side (left: the lower hull of (y, x), right: the upper one).  Returns the new length.
__device__ __forceinline__ int hull_push(int* seg, int n, int v, bool right) {
  const int px = hull_x(v), py = hull_y(v);
  while (n >= 2) {
    const int a = seg[n - 1], o = seg[n - 2];
    const long long cr = (long long)(hull_y(a) - hull_y(o)) * (px - hull_x(o)) - (long long)(hull_x(a) - hull_x(o)) * (py - hull_y(o));
    if (right ? cr < 0 : cr > 0) break;
    --n;
  }
  seg[n] = v;
  return n + 1;
}

__global__ __launch_bounds__(64) void hull_chain_kernel(HullPlanes p, int max_out) {
  __shared__ int s_count[64];
  __shared__ int s_pts[HULL_LDS_POINTS], s_lvl[HULL_LDS_POINTS];
  if (p.ctl[0]) return;
  const int lane = threadIdx.x;
  for (long u = blockIdx.x; u < 2L * max_out; u += gridDim.x) {      // uniform in the workgroup, which is one wave
    const int k = (int)(u >> 1);
    const bool right = u & 1;
    const int top = p.max_y[k];
    if (top < 0) continue;
    const int y0 = p.min_y[k], levels = top - y0 + 2, c = (levels + 63) >> 6;
    int* seg = (right ? p.right : p.left) + p.off[k];
    const int empty = right ? HULL_RIGHT_EMPTY : HULL_LEFT_EMPTY;
    const int lo = min(lane * c, levels), hi = min(lo + c, levels);
    int n = 0, mine = 0;
    const bool fits = levels <= HULL_LDS_POINTS;            // uniform: the first pass runs in LDS as well
    if (c == 1) {                                           // one level per lane: its point stays in a register
      if (lane < levels) {
        const int x = seg[lane];
        if (x != empty) n = 1, mine = hull_pack(x, y0 + lane);
      }
    } else if (fits) {
      for (int j = lane; j < levels; j += 64) s_lvl[j] = seg[j];     // coalesced
      __syncthreads();
      for (int j = lo; j < hi; ++j) {                       // writes s_lvl[lo + n], n <= j - lo: behind the read cursor
        const int x = s_lvl[j];
        if (x != empty) n = hull_push(s_lvl + lo, n, hull_pack(x, y0 + j), right);
      }
    } else {
      for (int j = lo; j < hi; ++j) {                       // the same in place in memory
        const int x = seg[j];
        if (x != empty) n = hull_push(seg + lo, n, hull_pack(x, y0 + j), right);
      }
    }
    const int incl = wave_incl_scan(n, lane);               // where this lane's points start in the concatenation
    const int total = __shfl(incl, 63, 64), at = incl - n;
    if (total <= HULL_LDS_POINTS) {                         // uniform: the second pass runs in LDS
      if (c == 1) {
        if (n) s_pts[at] = mine;
      } else if (fits) {
        for (int i = 0; i < n; ++i) s_pts[at + i] = s_lvl[lo + i];
      } else {
        for (int i = 0; i < n; ++i) s_pts[at + i] = seg[lo + i];
      }
      __syncthreads();
      if (lane == 0) {
        int m = 0;
        for (int i = 0; i < total; ++i) m = hull_push(s_pts, m, s_pts[i], right);    // writes s_pts[m], m <= i
        s_count[0] = m;
        p.count[u] = m;
      }
      __syncthreads();
      const int m = s_count[0];
      for (int i = lane; i < m; i += 64) seg[i] = s_pts[i];
    } else {                                                // more chunk vertices than LDS holds: the same pass in place in memory
      s_count[lane] = n;
      __syncthreads();                                      // the chunks' chains are in memory
      if (lane == 0) {
        int m = 0;
        for (int l = 0; l < 64; ++l) {
          const int nl = s_count[l], src = min(l * c, levels);
          for (int i = 0; i < nl; ++i) m = hull_push(seg, m, seg[src + i], right);   // writes seg[m], m <= src + i
        }
        p.count[u] = m;
      }
    }
    __syncthreads();
  }
}

// a (Wc, Wl) pair is better when Wc^2 / Wl is smaller, then when Wl is smaller; wl == 0 marks no edge
__device__ __forceinline__ bool hull_better(long long wc_a, int wl_a, long long wc_b, int wl_b) {
  if (wl_a == 0) return false;
  if (wl_b == 0) return true;
  const unsigned long long sa = (unsigned long long)(wc_a * wc_a), sb = (unsigned long long)(wc_b * wc_b);   // <= 2^58.1
  const unsigned long long ah = __umul64hi(sa, (unsigned long long)wl_b), al = sa * (unsigned long long)wl_b;
  const unsigned long long bh = __umul64hi(sb, (unsigned long long)wl_a), bl = sb * (unsigned long long)wl_a;
  if (ah != bh) return ah < bh;
  if (al != bl) return al < bl;
  return wl_a < wl_b;
}

__global__ __launch_bounds__(256) void hull_caliper_kernel(HullPlanes p, int max_out, long long* __restrict__ out) {
  if (p.ctl[0]) return;
  const int lane = threadIdx.x & 63;
  for (long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6); k < max_out; k += (long)gridDim.x * 4) {   // uniform within a wave
    if (p.max_y[k] < 0) continue;
    const int nl = p.count[2 * k], nv = nl + p.count[2 * k + 1];
    const int *left = p.left + p.off[k], *right = p.right + p.off[k];
    // the polygon: the left chain top to bottom, then the right chain bottom to top
    auto vert = [&](int i) { return i < nl ? left[i] : right[nv - 1 - i]; };
    long long area2 = 0, wc_best = 0;
    int f2 = 0, wl_best = 0;
    for (int i = lane; i < nv; i += 64) {
      const int a = vert(i), b = vert(i + 1 == nv ? 0 : i + 1);
      const int ax = hull_x(a), ay = hull_y(a), ex = hull_x(b) - ax, ey = hull_y(b) - ay;
      area2 += (long long)ax * hull_y(b) - (long long)hull_x(b) * ay;
      long long wc = 0;
      for (int j = 0; j < nv; ++j) {
        const int v = vert(j), dx = hull_x(v) - ax, dy = hull_y(v) - ay;
        const long long cr = (long long)ex * dy - (long long)ey * dx;
        wc = max(wc, cr < 0 ? -cr : cr);
        if (j > i) f2 = max(f2, dx * dx + dy * dy);         // <= 2 * 16384^2 = 2^29
      }
      const int wl = ex * ex + ey * ey;
      if (hull_better(wc, wl, wc_best, wl_best)) wc_best = wc, wl_best = wl;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      area2 += __shfl_xor(area2, o, 64);
      f2 = max(f2, __shfl_xor(f2, o, 64));
      const long long wc = __shfl_xor(wc_best, o, 64);
      const int wl = __shfl_xor(wl_best, o, 64);
      if (hull_better(wc, wl, wc_best, wl_best)) wc_best = wc, wl_best = wl;
    }
    if (lane == 0) {
      long long* o = out + k;
      const long r = max_out;
      o[H_H2 * r] = area2 < 0 ? -area2 : area2;
      o[H_F2 * r] = f2;
      o[H_WC * r] = wc_best;
      o[H_WL * r] = wl_best;
      o[H_NV * r] = nv;
    }
  }
}

int launch_label_hull(const int* label, int max_out, int h, int w, void* workspace, long workspace_bytes, long long* out,
                      int* out_rows, int max_rows, hipStream_t stream) {
  UNETDC_REQUIRE(label && workspace && out_rows && (out || max_out == 0), "label_hull: null pointer");
  const auto lay = hull_layout(h, w, max_out, max_rows, workspace);
  UNETDC_REQUIRE(lay.ok, "label_hull: bad geometry (sides 1..16384, non-negative label limit, row limit 0..2^28)");
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "label_hull: workspace must be 4-byte aligned");
  if (int rc = require_workspace("label_hull", workspace_bytes, lay.bytes)) return rc;
  const HullPlanes& p = lay.planes;
  const int rows_grid = grid_for((long)h * ((w + 63) / 64), 4);
  hipLaunchKernelGGL(hull_init_kernel, dim3(grid_for((long)HULL_QUANTITIES * max_out, 256, 1024)), dim3(256), 0, stream, p, max_out, out);
  hipLaunchKernelGGL(hull_extent_kernel, dim3(rows_grid), dim3(256), 0, stream, label, max_out, h, w, p);
  hipLaunchKernelGGL(hull_scan_kernel, dim3(1), dim3(1024), 0, stream, p, max_out, max_rows, out_rows);
  hipLaunchKernelGGL(hull_fill_kernel, dim3(grid_for(p.slots, 256, 1024)), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(hull_rows_kernel, dim3(rows_grid), dim3(256), 0, stream, label, max_out, h, w, p);
  hipLaunchKernelGGL(hull_chain_kernel, dim3(grid_for(2L * max_out, 1, HULL_MAX_CHAINS)), dim3(64), 0, stream, p, max_out);
  hipLaunchKernelGGL(hull_caliper_kernel, dim3(grid_for(max_out, 4, HULL_MAX_GROUPS)), dim3(256), 0, stream, p, max_out, out);
  return check_launch("label_hull kernels");
}

}  // namespace unetdc
