// Droplets per cell ("Droplets per cell"): the exact nearest-label transform of a seed label map (the territories of
// nuclei) and the per-cell reduction of the droplet table.  All integer work, defined pixel by pixel: no result depends on the
// order in which anything runs (bitwise reproducible, equal to utils/droplet_cells.py).
//
// unetdc_label_nearest: for every pixel the lexicographic minimum over the seed pixels q of (|p - q|^2, label[q]).  Separable:
//   nearest_col_kernel    (g, gl)[y][x] = the minimum (dy, label) over the seeds of column x (CELL_NONE, 0 without one): one
//                         thread per column walks down with the last seed above, then up with the last seed below; the nearer
//                         one wins, at equal dy the smaller label.  Neighbouring threads read neighbouring words.  Serial over h.
//   nearest_row_kernel    (D2, L)[y][x] = the minimum over x' of ((x - x')^2 + g[y][x']^2, gl[y][x']): (x - x')^2 is constant
//                         within a column, so the minimum of the column composes.  One workgroup per row, both planes of the row
//                         in LDS (8 w bytes: 128 KiB at w = 16384, asked for with the dynamic-LDS attribute), every thread
//                         scans outward from x WHILE dx^2 <= the best distance so far: a candidate at dx^2 == best with column
//                         distance 0 ties on distance and may carry a smaller label (edt_row_kernel of split.hip stops at
//                         dx^2 >= best, which is right for the distance alone).  The label plane is read only where the distance
//                         does not lose.  A row without any finite g (then no row has one) gets (UNETDC_EDT_INF, 0) after one
//                         workgroup-wide vote.  The radius cuts the label at the store; the distance stays exact.
//
// unetdc_cell_table: the droplet label map against the cell label map.
//   cells_init_kernel     every output row at its initial value, the per-droplet argmax words 0
//   pair_init_kernel      (pair_table.h) the (droplet, cell) table empty
//   cells_pixel_kernel    one wave per 64 consecutive pixels of a row, as match_overlap_kernel.  Three run decompositions
//                         (wave_runs, wave_ops.h), each reduced inside the wave so that only run heads issue atomics: by droplet
//                         (area, pixels on no cell, minimum d2), by cell (area, border, droplet pixels, d2 == 0 pixels) and by
//                         (droplet, cell), whose head inserts the run length into the pair table
//   pair_compact / pair_sort_* / pair_emit   (pair_table.h) the sorted triples (droplet, cell, n), *out_needed
//   cells_argmax_kernel   over the sorted triples: n_cells by atomic add, the argmax by a 64-bit atomic max on
//                         (n << 32) | ~cell: the largest n, at equal n the smallest cell
//   cells_assign_kernel   per droplet: the argmax word -> cell, n_in; a droplet with a cell adds itself to that cell's
//                         n_droplets, S_area, S_area2 and max_area (64-bit integer atomics: any order gives the same sums)
#include "pair_table.h"
#include "wave_ops.h"

namespace unetdc {

constexpr int CELL_NONE = 0x7fffffff;             // g: no seed in this column
constexpr int CELLS_MAX_SIDE = 16384;             // d2 <= 2 * 16383^2 < 2^30; both planes of a row fit 128 KiB of LDS
constexpr int CELLS_MAX_RADIUS = 32767;

// ---- nearest label ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void nearest_col_kernel(const int* __restrict__ label, int max_label, int* __restrict__ g,
                                                         int* __restrict__ gl, int h, int w) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  int d = CELL_NONE, l = 0;
#pragma unroll 4
  for (int y = 0; y < h; ++y) {
    const long i = (long)y * w + x;
    const int v = label[i];
    if (v >= 1 && v <= max_label) d = 0, l = v;
    else if (d != CELL_NONE) ++d;
    g[i] = d;
    gl[i] = l;
  }
  d = CELL_NONE, l = 0;
#pragma unroll 4
  for (int y = h - 1; y >= 0; --y) {
    const long i = (long)y * w + x;
    const int v = label[i];
    if (v >= 1 && v <= max_label) d = 0, l = v;
    else if (d != CELL_NONE) ++d;
    const int gd = g[i];
    if (d < gd || (d == gd && d != CELL_NONE && l < gl[i])) {
      g[i] = d;
      gl[i] = l;
    }
  }
}

__global__ __launch_bounds__(256) void nearest_row_kernel(const int* __restrict__ g, const int* __restrict__ gl,
                                                          int* __restrict__ out_label, int* __restrict__ out_d2, int w,
                                                          long long r2) {
  extern __shared__ int row[];                               // [w] column distances, then [w] column labels
  int* rowl = row + w;
  const long base = (long)blockIdx.x * w;
  int finite = 0;
  for (int x = threadIdx.x; x < w; x += 256) {
    const int v = g[base + x];
    row[x] = v;
    rowl[x] = gl[base + x];
    finite |= v != CELL_NONE;
  }
  if (!__syncthreads_or(finite)) {                           // also the barrier that publishes row[] and rowl[]
    for (int x = threadIdx.x; x < w; x += 256) {
      out_d2[base + x] = UNETDC_EDT_INF;
      out_label[base + x] = 0;
    }
    return;
  }
  for (int x = threadIdx.x; x < w; x += 256) {
    const int g0 = row[x];
    int best = g0 == CELL_NONE ? UNETDC_EDT_INF : g0 * g0, bl = g0 == CELL_NONE ? 0 : rowl[x];
    // dx <= 16383: dx^2 < 2^28, and a finite candidate is below 2^29
    for (int dx = 1; dx * dx <= best; ++dx) {
      const int l = x - dx, r = x + dx, dd = dx * dx;
      if (l < 0 && r >= w) break;
      if (l >= 0) {
        const int v = row[l];
        if (v != CELL_NONE) {
          const int c = dd + v * v;
          if (c <= best) {
            const int cl = rowl[l];
            if (c < best || cl < bl) best = c, bl = cl;
          }
        }
      }
      if (r < w) {
        const int v = row[r];
        if (v != CELL_NONE) {
          const int c = dd + v * v;
          if (c <= best) {
            const int cl = rowl[r];
            if (c < best || cl < bl) best = c, bl = cl;
          }
        }
      }
    }
    out_d2[base + x] = best;
    out_label[base + x] = (r2 > 0 && (long long)best > r2) ? 0 : bl;
  }
}

struct NearestPlanes {
  int* g;    // [h * w] column distance
  int* gl;   // [h * w] column label
};
static Layout<NearestPlanes> nearest_layout(int h, int w, void* workspace) {
  if (!(h >= 1 && w >= 1 && h <= CELLS_MAX_SIDE && w <= CELLS_MAX_SIDE)) return {false, 0, {}};
  const long n = (long)h * w;
  Carver c(workspace);
  NearestPlanes p;
  p.g = c.take<int>(n, 64);
  p.gl = c.take<int>(n, 64);
  return {true, c.bytes(), p};
}
long label_nearest_workspace_bytes(int h, int w) { return nearest_layout(h, w, nullptr).bytes; }

int launch_label_nearest(const int* label, int max_label, int h, int w, int radius, void* workspace, long workspace_bytes,
                         int* out_label, int* out_d2, hipStream_t stream) {
  UNETDC_REQUIRE(label && workspace && out_label && out_d2, "label_nearest: null pointer");
  const auto lay = nearest_layout(h, w, workspace);
  UNETDC_REQUIRE(lay.ok && radius >= 0 && radius <= CELLS_MAX_RADIUS && max_label >= 0,
                 "label_nearest: bad geometry (sides 1..16384, radius 0..32767, non-negative label limit)");
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "label_nearest: workspace must be 4-byte aligned");
  if (int rc = require_workspace("label_nearest", workspace_bytes, lay.bytes)) return rc;
  const int lds = w * 8;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&nearest_row_kernel), lds, "nearest_row_kernel")) return rc;
  const auto [g, gl] = lay.planes;
  hipLaunchKernelGGL(nearest_col_kernel, dim3((w + 63) / 64), dim3(64), 0, stream, label, max_label, g, gl, h, w);
  hipLaunchKernelGGL(nearest_row_kernel, dim3(h), dim3(256), (size_t)lds, stream, g, gl, out_label, out_d2, w,
                     (long long)radius * radius);
  return check_launch("label nearest kernels");
}

// ---- per-cell table -----------------------------------------------------------------------------------------------------------

enum { CD_CELL = 0, CD_N_IN, CD_N_CELLS, CD_N_OUT, CD_AREA, CD_MIN_D2 };
enum { CC_AREA = 0, CC_N_BORDER, CC_FG_PX, CC_N_DROPLETS, CC_S_AREA, CC_S_AREA2, CC_MAX_AREA, CC_NUCLEUS_PX };
static_assert(CD_MIN_D2 + 1 == CELL_DROPLET_QUANTITIES && CC_NUCLEUS_PX + 1 == CELL_QUANTITIES, "unetdc_cell_table output rows");

struct CellPlanes {
  PairPlanes p;
  unsigned long long* best;   // [max_droplet] (n << 32) | ~cell of the droplet's best triple so far, 0 = none
  int *ta, *tb, *tn;          // [pairs] the sorted triples
};
// the pair table (at most h * w triples, and none without a droplet or without a cell), the argmax words and the triples.
// max_cell has no plane of its own: the per-cell sums go straight to the output.
static Layout<CellPlanes> cells_layout(int h, int w, int max_droplet, int max_cell, int max_pairs, void* workspace) {
  if (!(h >= 1 && w >= 1 && h <= CELLS_MAX_SIDE && w <= CELLS_MAX_SIDE && max_droplet >= 0 && max_cell >= 0 && max_pairs >= 0))
    return {false, 0, {}};
  Carver c(workspace);
  CellPlanes s;
  s.p = pair_carve(c, (int)std::min((long)max_pairs, (long)h * w));
  s.best = c.take<unsigned long long>(max_droplet, 64);
  s.ta = c.take<int>(s.p.max_pairs, 64);
  s.tb = c.take<int>(s.p.max_pairs, 64);
  s.tn = c.take<int>(s.p.max_pairs, 64);
  return {true, c.bytes(), s};
}
long cell_table_workspace_bytes(int h, int w, int max_droplet, int max_cell, int max_pairs) {
  return cells_layout(h, w, max_droplet, max_cell, max_pairs, nullptr).bytes;
}

__global__ void cells_init_kernel(unsigned long long* __restrict__ best, int* __restrict__ out_droplet, int max_droplet,
                                  long long* __restrict__ out_cell, int max_cell) {
  const int stride = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
  for (int k = t; k < max_droplet; k += stride) {
    best[k] = 0ull;
#pragma unroll
    for (int j = 0; j < CELL_DROPLET_QUANTITIES; ++j) out_droplet[(long)j * max_droplet + k] = j == CD_MIN_D2 ? UNETDC_EDT_INF : 0;
  }
  for (long k = t; k < (long)CELL_QUANTITIES * max_cell; k += stride) out_cell[k] = 0;
}

__global__ __launch_bounds__(256) void cells_pixel_kernel(const int* __restrict__ droplet_label, int max_droplet,
                                                          const int* __restrict__ cell_label, int max_cell,
                                                          const int* __restrict__ d2, int h, int w, PairPlanes p,
                                                          int* __restrict__ out_droplet, long long* __restrict__ out_cell) {
  const int lane = threadIdx.x & 63;
  const int chunks = (w + 63) >> 6;
  const long units = (long)h * chunks;
  const long stride = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += stride) {   // uniform within a wave
    const RowUnit px = row_unit(u, chunks, w, lane);
    int a = px.in ? droplet_label[px.i] : 0, b = px.in ? cell_label[px.i] : 0;
    // labels below 1 or above the given maxima are background
    if (a < 1 || a > max_droplet) a = 0;
    if (b < 1 || b > max_cell) b = 0;
    if (__ballot((a | b) != 0) == 0ull) continue;            // wave-uniform: background on both maps
    const int d = (d2 && px.in) ? d2[px.i] : UNETDC_EDT_INF;
    {
      const WaveRuns r = wave_runs(a, lane);
      const int n = r.len, n_out = run_sum<int>(b == 0, r, lane), dmin = run_min<int>(d, r, lane);
      if (a != 0 && r.head) {
        atomicAdd(out_droplet + (long)CD_AREA * max_droplet + a - 1, n);
        if (n_out) atomicAdd(out_droplet + (long)CD_N_OUT * max_droplet + a - 1, n_out);
        if (dmin != UNETDC_EDT_INF) atomicMin(out_droplet + (long)CD_MIN_D2 * max_droplet + a - 1, dmin);
      }
    }
    {
      const WaveRuns r = wave_runs(b, lane);
      const bool border = px.y == 0 || px.y == h - 1 || px.x == 0 || px.x == w - 1;
      const int n = r.len, n_border = run_sum<int>(border, r, lane), fg = run_sum<int>(a != 0, r, lane),
                nucleus = run_sum<int>(d == 0, r, lane);
      if (b != 0 && r.head) {
        atomic_add64(out_cell + (long)CC_AREA * max_cell + b - 1, n);
        if (n_border) atomic_add64(out_cell + (long)CC_N_BORDER * max_cell + b - 1, n_border);
        if (fg) atomic_add64(out_cell + (long)CC_FG_PX * max_cell + b - 1, fg);
        if (nucleus) atomic_add64(out_cell + (long)CC_NUCLEUS_PX * max_cell + b - 1, nucleus);
      }
    }
    {
      const pair_key_t key = (a != 0 && b != 0) ? ((pair_key_t)(unsigned)a << 32) | (unsigned)b : 0ull;
      const WaveRuns r = wave_runs(key, lane);
      if (key != 0ull && r.head) pair_insert<PairAdd>(p, key, r.len);
    }
  }
}

__global__ void cells_argmax_kernel(CellPlanes s, int max_droplet, int* __restrict__ out_droplet) {
  const int entries = s.p.ctl[PAIR_ENTRIES];
  const int m = entries < s.p.max_pairs ? entries : s.p.max_pairs;      // real keys: their labels are in range
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const int a = s.ta[i], b = s.tb[i], n = s.tn[i];
    atomicAdd(out_droplet + (long)CD_N_CELLS * max_droplet + a - 1, 1);
    atomicMax(s.best + a - 1, ((unsigned long long)(unsigned)n << 32) | (unsigned)~b);
  }
}

__global__ void cells_assign_kernel(const unsigned long long* __restrict__ best, int* __restrict__ out_droplet, int max_droplet,
                                    long long* __restrict__ out_cell, int max_cell) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < max_droplet; k += gridDim.x * blockDim.x) {
    const unsigned long long v = best[k];
    if (v == 0ull) continue;                                 // cell and n_in keep their zeros
    const int cell = (int)~(unsigned)(v & 0xffffffffull), n_in = (int)(v >> 32);
    out_droplet[(long)CD_CELL * max_droplet + k] = cell;
    out_droplet[(long)CD_N_IN * max_droplet + k] = n_in;
    const long long area = out_droplet[(long)CD_AREA * max_droplet + k];
    atomic_add64(out_cell + (long)CC_N_DROPLETS * max_cell + cell - 1, 1);
    atomic_add64(out_cell + (long)CC_S_AREA * max_cell + cell - 1, area);
    atomic_add64(out_cell + (long)CC_S_AREA2 * max_cell + cell - 1, area * area);
    atomicMax(reinterpret_cast<unsigned long long*>(out_cell + (long)CC_MAX_AREA * max_cell + cell - 1), (unsigned long long)area);
  }
}

int launch_cell_table(const int* droplet_label, int max_droplet, const int* cell_label, int max_cell, const int* d2, int h, int w,
                      void* workspace, long workspace_bytes, int* out_needed, int max_pairs, int* out_droplet, long long* out_cell,
                      hipStream_t stream) {
  UNETDC_REQUIRE(droplet_label && cell_label && workspace && out_needed && (out_droplet || max_droplet <= 0) &&
                     (out_cell || max_cell <= 0),
                 "cell_table: null pointer");
  const auto lay = cells_layout(h, w, max_droplet, max_cell, max_pairs, workspace);
  UNETDC_REQUIRE(lay.ok, "cell_table: bad geometry (sides 1..16384, non-negative label and pair limits)");
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(out_cell) & 7) == 0,
                 "cell_table: workspace and out_cell must be 8-byte aligned");
  if (int rc = require_workspace("cell_table", workspace_bytes, lay.bytes)) return rc;
  const CellPlanes& s = lay.planes;
  const long rows = std::max((long)max_droplet, (long)CELL_QUANTITIES * max_cell);
  hipLaunchKernelGGL(cells_init_kernel, dim3(grid_for(rows, 256, 2048)), dim3(256), 0, stream, s.best, out_droplet, max_droplet,
                     out_cell, max_cell);
  pair_table_init<PairAdd>(s.p, stream);
  const long units = (long)h * ((w + 63) / 64);
  hipLaunchKernelGGL(cells_pixel_kernel, dim3(grid_for(units, 4, 8192)), dim3(256), 0, stream, droplet_label, max_droplet,
                     cell_label, max_cell, d2, h, w, s.p, out_droplet, out_cell);
  pair_table_list(s.p, max_pairs, out_needed, s.ta, s.tb, s.tn, stream);
  hipLaunchKernelGGL(cells_argmax_kernel, dim3(grid_for(s.p.max_pairs, 256, 2048)), dim3(256), 0, stream, s, max_droplet,
                     out_droplet);
  hipLaunchKernelGGL(cells_assign_kernel, dim3(grid_for(max_droplet, 256, 2048)), dim3(256), 0, stream, s.best, out_droplet,
                     max_droplet, out_cell, max_cell);
  return check_launch("cell table kernels");
}

}  // namespace unetdc
