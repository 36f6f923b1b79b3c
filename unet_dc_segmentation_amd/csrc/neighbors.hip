// Droplet neighbourhoods of an int32 label map: the pairs of labels whose smallest squared pixel
// distance is at most radius^2, in ascending order of (a, b), and per label its nearest contact, degree and cluster.
// Integer work only; the order of the pair list is fixed by a sort on unique keys: two runs give the same bytes.
//
//   pair_init_kernel          (pair_table.h) the table empty, distances at INT_MAX, the control words 0
//   neighbors_init_kernel     per label: nearest word all ones, parent = itself, present 0, size 0, degree 0
//   neighbors_border_kernel   one wave per tile of 16 rows x 64 columns.  A pixel takes part if its label is in range and an
//                             in-image 4-neighbour carries another value (the minimum over a pair is always reached at such a
//                             pixel: from any other pixel one step towards the partner stays in the label and is closer).
//                             One ballot per row and ONE atomic add per tile append the linear indices to the list (every
//                             append meets on one counter: with one atomic per row of 64 pixels the kernel took 75 us on a
//                             1040 x 1388 droplet map); its order is arrival order and nothing below depends on it.  Run
//                             heads mark their label present.
//   neighbors_scan_kernel     one wave per border pixel p of label a.  The lanes run over the columns x - G .. x + G (64 per
//                             trip), the rows over -G .. G cut to the image; a lane reads label(q) only where
//                             dx^2 + dy^2 <= G^2 and q is inside the image, and a row whose lanes of this trip all lie outside
//                             the disc is skipped.  label(q) > a in range is a hit: each unordered pair is found from the
//                             smaller label's side.  A lane keeps its last partner and running minimum down its column and
//                             inserts only when the partner changes and at the end.  The label map is read from global memory
//                             (L2): the row segments are coalesced and neighbouring border pixels read the same lines.
//   pair_compact / pair_sort_* / pair_emit   (pair_table.h) the table -> the sorted list, the outputs, *out_count
//   neighbors_pairs_kernel    over the sorted list: degree by atomic add, nearest by a 64-bit atomic min on (d2 << 32) | other,
//                             clusters by ccl_unite on the parent array over the labels (the root is the smallest label)
//   neighbors_flatten_kernel  cluster = ccl_find; present labels count into size[root]; nearest word -> nn_label, nn_d2
//   neighbors_size_kernel     cluster_size = size[cluster] for a present label, else 0
#include "ccl_uf.h"
#include "pair_table.h"

namespace unetdc {

enum { NEIGHBORS_BORDER = PAIR_USER };         // control word: the length of the border list

struct NeighborPlanes {
  int* border;                   // [h * w] linear indices of the border pixels
  unsigned long long* nearest;   // [max_label + 1] (d2 << 32) | other, all ones = none
  int* parent;                   // [max_label + 1]
  int* present;                  // [max_label + 1]
  int* size;                     // [max_label + 1]
};

// a label has at most max_label - 1 partners; 2^27 pairs is the largest table (3 GB) the int32 planes are sized for
static int neighbors_effective_pairs(int max_label, int max_pairs) {
  long n = (long)max_label * (max_label - 1) / 2;
  if (n < 0) n = 0;
  if (n > (1L << 27)) n = 1L << 27;
  return (long)max_pairs < n ? max_pairs : (int)n;
}

// the pair table, then the per-label planes (each the int32 plane of max_label + 1 words rounded to 64 bytes; nearest twice
// that) and the border list, rounded to 64 bytes too.  The radius is the launcher's own check: the layout does not depend on it.
struct NeighborsWorkspace {
  PairPlanes p;
  NeighborPlanes q;
};
static Layout<NeighborsWorkspace> neighbors_layout(int h, int w, int max_label, int max_pairs, void* workspace) {
  if (!(h > 0 && w > 0 && h <= 16384 && w <= 16384 && max_label >= 0 && max_pairs >= 0)) return {false, 0, {}};
  const long words = align_up(((long)max_label + 1) * 4, 64) / 4;
  Carver c(workspace);
  NeighborsWorkspace s;
  s.p = pair_carve(c, neighbors_effective_pairs(max_label, max_pairs));
  s.q.nearest = c.take<unsigned long long>(words);
  s.q.parent = c.take<int>(words);
  s.q.present = c.take<int>(words);
  s.q.size = c.take<int>(words);
  s.q.border = c.take<int>((long)h * w, 64);
  return {true, c.bytes(), s};
}
long label_neighbors_workspace_bytes(int h, int w, int max_label, int max_pairs) {
  return neighbors_layout(h, w, max_label, max_pairs, nullptr).bytes;
}

__global__ void neighbors_init_kernel(NeighborPlanes q, int max_label, int* __restrict__ out_degree) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k <= max_label; k += gridDim.x * blockDim.x) {
    q.nearest[k] = ~0ull;
    q.parent[k] = k;
    q.present[k] = 0;
    q.size[k] = 0;
    if (k > 0) out_degree[k - 1] = 0;
  }
}

constexpr int NEIGHBORS_TILE_ROWS = 16;        // rows of the 64-column tile one wave of neighbors_border_kernel owns

__global__ __launch_bounds__(256) void neighbors_border_kernel(const int* __restrict__ label, int max_label, int h, int w,
                                                               NeighborPlanes q, int* __restrict__ ctl) {
  constexpr int R = NEIGHBORS_TILE_ROWS;
  const int lane = threadIdx.x & 63;
  const int chunks = (w + 63) >> 6;
  const long units = (long)((h + R - 1) / R) * chunks;
  const long stride = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += stride) {   // uniform within a wave
    const int ty = (int)(u / chunks), x = ((int)(u - (long)ty * chunks) << 6) + lane;
    const int y0 = ty * R;
    const bool in = x < w;
    int v[R + 2];                                            // the tile's column with the row above and the row below
#pragma unroll
    for (int r = 0; r < R + 2; ++r) {
      const int yy = y0 - 1 + r;                             // uniform: rows outside the image are never read
      v[r] = in && yy >= 0 && yy < h ? label[yy * w + x] : 0;               // h * w <= 2^28
    }
    unsigned long long m[R];
    int total = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int y = y0 + r, a = v[r + 1];
      const bool fg = y < h && a > 0 && a <= max_label;      // labels below 1 or above max_label take no part
      const int left = __shfl_up(a, 1, 64), right = __shfl_down(a, 1, 64);
      bool edge = false;
      if (fg) {
        const int i = y * w + x;
        if (x > 0) edge |= (lane > 0 ? left : label[i - 1]) != a;
        if (x + 1 < w) edge |= (lane < 63 ? right : label[i + 1]) != a;
        if (y > 0) edge |= v[r] != a;
        if (y + 1 < h) edge |= v[r + 2] != a;
        // run heads; every writer stores the same value, and only until the first store is seen
        if ((lane == 0 || left != a) && !*reinterpret_cast<volatile int*>(q.present + a)) q.present[a] = 1;
      }
      m[r] = __ballot(edge);
      total += __popcll(m[r]);
    }
    if (total == 0) continue;                                // wave-uniform
    int base = 0;
    if (lane == 0) base = atomicAdd(ctl + NEIGHBORS_BORDER, total);         // one atomic per tile: they all meet on one word
    base = __shfl(base, 0, 64);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if ((m[r] >> lane) & 1ull) q.border[base + __popcll(m[r] & ((1ull << lane) - 1ull))] = (y0 + r) * w + x;
      base += __popcll(m[r]);
    }
  }
}

__global__ __launch_bounds__(256) void neighbors_scan_kernel(const int* __restrict__ label, int max_label, int h, int w, int G,
                                                             NeighborPlanes q, PairPlanes p) {
  const int lane = threadIdx.x & 63;
  const int n = p.ctl[NEIGHBORS_BORDER];
  const int G2 = G * G, trips = (2 * G + 1 + 63) >> 6;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {        // uniform within a wave
    const int pix = q.border[i];
    const int y = pix / w, x = pix - y * w;
    const int a = label[pix];
    const pair_key_t hi = (pair_key_t)(unsigned)a << 32;
    const int y0 = y - G > 0 ? y - G : 0, y1 = y + G < h - 1 ? y + G : h - 1;
    for (int t = 0; t < trips; ++t) {
      const int lo = -G + (t << 6), last_dx = lo + 63 < G ? lo + 63 : G;          // this trip's columns, relative
      if (x + last_dx < 0 || x + lo >= w) continue;                               // wholly outside the image
      const int near = lo > 0 ? lo : last_dx < 0 ? -last_dx : 0;                  // the smallest |dx| of the trip
      const int dx = lo + lane, xx = x + dx;
      const bool col = dx <= G && xx >= 0 && xx < w;
      const int dx2 = dx * dx;
      int other = 0, best = 0;
      for (int yy = y0; yy <= y1; ++yy) {
        const int dy2 = (yy - y) * (yy - y);
        if (near * near + dy2 > G2) continue;                                     // no lane of this trip is in the disc
        const int d2 = dx2 + dy2;
        const int b = col && d2 <= G2 ? label[yy * w + xx] : 0;                   // never read outside the image
        if (b > a && b <= max_label) {
          if (b != other) {
            if (other) pair_insert<PairMin>(p, hi | (unsigned)other, best);
            other = b;
            best = d2;
          } else if (d2 < best) {
            best = d2;
          }
        }
      }
      if (other) pair_insert<PairMin>(p, hi | (unsigned)other, best);
    }
  }
}

__global__ void neighbors_pairs_kernel(PairPlanes p, NeighborPlanes q, int* __restrict__ out_degree) {
  const int entries = p.ctl[PAIR_ENTRIES];
  const int m = entries < p.max_pairs ? entries : p.max_pairs;          // real keys: their labels are in range
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const pair_key_t k = p.ek[i];
    const int a = (int)(k >> 32), b = (int)(k & 0xffffffffull);
    const unsigned long long d = (unsigned long long)(unsigned)p.ev[i] << 32;
    atomicAdd(out_degree + a - 1, 1);
    atomicAdd(out_degree + b - 1, 1);
    atomicMin(q.nearest + a, d | (unsigned)b);
    atomicMin(q.nearest + b, d | (unsigned)a);
    ccl_unite(q.parent, a, b);
  }
}

__global__ void neighbors_flatten_kernel(NeighborPlanes q, int max_label, int* __restrict__ out_nn_label,
                                         int* __restrict__ out_nn_d2, int* __restrict__ out_cluster) {
  for (int k = 1 + blockIdx.x * blockDim.x + threadIdx.x; k <= max_label; k += gridDim.x * blockDim.x) {
    const int root = ccl_find(q.parent, k);
    out_cluster[k - 1] = root;
    if (q.present[k]) atomicAdd(q.size + root, 1);
    const unsigned long long nn = q.nearest[k];
    out_nn_label[k - 1] = nn == ~0ull ? 0 : (int)(nn & 0xffffffffull);
    out_nn_d2[k - 1] = nn == ~0ull ? UNETDC_EDT_INF : (int)(nn >> 32);
  }
}

__global__ void neighbors_size_kernel(NeighborPlanes q, int max_label, const int* __restrict__ out_cluster,
                                      int* __restrict__ out_cluster_size) {
  for (int k = 1 + blockIdx.x * blockDim.x + threadIdx.x; k <= max_label; k += gridDim.x * blockDim.x)
    out_cluster_size[k - 1] = q.present[k] ? q.size[out_cluster[k - 1]] : 0;
}

int launch_label_neighbors(const int* label, int max_label, int h, int w, int radius, void* workspace, long workspace_bytes,
                           int* out_count, int* out_a, int* out_b, int* out_d2, int max_pairs, int* out_nn_label,
                           int* out_nn_d2, int* out_degree, int* out_cluster, int* out_cluster_size, hipStream_t stream) {
  UNETDC_REQUIRE(label && workspace && out_count && ((out_a && out_b && out_d2) || max_pairs <= 0) &&
                     ((out_nn_label && out_nn_d2 && out_degree && out_cluster && out_cluster_size) || max_label <= 0),
                 "label_neighbors: null pointer");
  const auto lay = neighbors_layout(h, w, max_label, max_pairs, workspace);
  UNETDC_REQUIRE(lay.ok && radius >= 1 && radius <= 64,
                 "label_neighbors: bad geometry (sides 1..16384, radius 1..64, non-negative label and pair limits)");
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "label_neighbors: workspace must be 8-byte aligned");
  if (int rc = require_workspace("label_neighbors", workspace_bytes, lay.bytes)) return rc;
  const PairPlanes& p = lay.planes.p;
  const NeighborPlanes& q = lay.planes.q;
  const int label_grid = grid_for((long)max_label + 1, 256, 2048);
  pair_table_init<PairMin>(p, stream);
  hipLaunchKernelGGL(neighbors_init_kernel, dim3(label_grid), dim3(256), 0, stream, q, max_label, out_degree);
  const long units = (long)((h + NEIGHBORS_TILE_ROWS - 1) / NEIGHBORS_TILE_ROWS) * ((w + 63) / 64);
  hipLaunchKernelGGL(neighbors_border_kernel, dim3(grid_for(units, 4, 8192)), dim3(256), 0, stream, label, max_label, h, w, q,
                     p.ctl);
  hipLaunchKernelGGL(neighbors_scan_kernel, dim3(grid_for((long)h * w, 4, 4096)), dim3(256), 0, stream, label, max_label, h, w,
                     radius, q, p);
  pair_table_list(p, max_pairs, out_count, out_a, out_b, out_d2, stream);
  hipLaunchKernelGGL(neighbors_pairs_kernel, dim3(grid_for(p.max_pairs, 256, 2048)), dim3(256), 0, stream, p, q, out_degree);
  hipLaunchKernelGGL(neighbors_flatten_kernel, dim3(label_grid), dim3(256), 0, stream, q, max_label, out_nn_label, out_nn_d2,
                     out_cluster);
  hipLaunchKernelGGL(neighbors_size_kernel, dim3(label_grid), dim3(256), 0, stream, q, max_label, out_cluster, out_cluster_size);
  return check_launch("label neighbors kernels");
}

}  // namespace unetdc
