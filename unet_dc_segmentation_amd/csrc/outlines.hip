// Ordered outlines of every droplet of an int32 label map: crack-following contours as list ranking over boundary edges
// (the rule is stated once in utils/droplet_outlines.py).  A crack is a unit edge between a pixel of
// label k and a pixel that is not k, directed with the k-pixel on its right; its id is (tail corner) * 4 + direction.  Every
// crack has one successor, so the cracks of a label are disjoint cycles: the contours.
//
// The census runs over the lattice CORNERS, not the pixels: the (up to four) cracks that leave a corner have consecutive ids,
// so numbering them corner by corner puts all cracks in ascending id order, and "the crack of smallest id" of a cycle is the
// one of smallest index.  (In pixel order the top crack of pixel (r, c + 1) would come behind the right crack of (r, c), whose
// id is larger.)
//
//   ol_init_kernel          out rows, needed[4] and the control words: zeros
//   ol_census_kernel        per tile of 1024 corners: the number of cracks that leave them (4 pixels read per corner)
//   ol_scan_cracks_kernel   one workgroup: exclusive scan of the tile counts; needed[0]; the overflow flag
//   ol_base_kernel          the same tiles again: every corner's index of its first crack
//   ol_successor_kernel     per corner and crack: the successor rule at the head, the successor's index (its corner's base +
//                           the popcount of the lower directions there), the turn flag, the shoelace term
//   ol_leader_kernel        r = ceil(log2(max_len)) launches: (jump, min) -> (jump o jump, min of the two windows), ping-pong
//   ol_cut_kernel           leader[i] != leader[next[i]] anywhere: a cycle longer than 2^r, flag; else every cycle is cut in front
//                           of its leader (next = -1 there) and the ranks start as (1, turn, term)
//   ol_rank_kernel          r launches: suffix sums of the three weights by pointer jumping, ping-pong.  At a leader they are
//                           the contour's length, vertex count and signed area; elsewhere what lies from the crack to the end
//   ol_contour_count_kernel per tile of 1024 cracks: leaders, and their vertices; a contour longer than max_len: flag
//   ol_scan_contours_kernel one workgroup: both scans; needed[1], needed[2], needed[3]
//   ol_contours_kernel      the tiles again: a leader's place is its contour's index (ascending start id), the vertex prefix its
//                           `first`; the contour table where it fits; five integer atomic adds per contour into the label's rows
//   ol_vertices_kernel      per turning crack: vertex (turns before it + 1) mod nv of its contour is its head
// No launch reads what another workgroup writes in the same launch; nothing waits on another workgroup.  Integer atomic adds and
// fixed-order scans only: bitwise reproducible.
#include "kernels.h"
#include "wave_ops.h"
#include "workspace.h"

namespace unetdc {

enum { O_E = 0, O_NO, O_NH, O_NV, O_F2, O_S2 };
static_assert(O_S2 + 1 == OUTLINE_QUANTITIES, "outline quantities");
enum { C_LABEL = 0, C_FIRST, C_NV, C_LENGTH, C_S2 };
static_assert(C_S2 + 1 == CONTOUR_FIELDS, "contour fields");
enum { OL_N = 0, OL_OVER, OL_LONG, OL_LEN };   // ctl: cracks (0 when they do not fit), cracks > room, cycle > 2^r or merged, contour > max_len

constexpr int OL_THREADS = 256, OL_ITEMS = 4, OL_TILE = OL_THREADS * OL_ITEMS;
constexpr int OL_MAX_GRID = 4096;

struct OutlinePlanes {
  int* ctl;                       // [16]
  int* base;                      // [corners] index of the first crack that leaves the corner
  int *tile_cracks, *tile_base;   // [corner tiles] cracks of a tile, and their exclusive scan
  int *tile_n[2], *tile_at[2];    // [crack tiles] leaders / their vertices of a tile, and the exclusive scans
  int *next, *leader;             // [max_cracks]
  unsigned* where;                // [max_cracks] tail corner << 3 | direction << 1 | turn
  int *jump[2], *val[2], *turns[2];   // [max_cracks] ping-pong: (jump, min index), then (next, length, turns)
  long long* area[2];             // [max_cracks] ping-pong: the shoelace sums
  long corners;
  int corner_tiles, crack_tiles;
};

static Layout<OutlinePlanes> outline_layout(int h, int w, int max_out, int max_cracks, void* workspace) {
  if (!(h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30) && max_out >= 0 && max_cracks >= 0 && max_cracks <= (1 << 30))) return {false, 0, {}};
  Carver c(workspace);
  OutlinePlanes p;
  p.corners = (long)(h + 1) * (w + 1);                      // < 2^29
  p.corner_tiles = (int)((p.corners + OL_TILE - 1) / OL_TILE);
  p.crack_tiles = (int)(((long)max_cracks + OL_TILE - 1) / OL_TILE);
  const long m = max_cracks;
  p.ctl = c.take<int>(16, 64);
  p.base = c.take<int>(p.corners, 64);
  p.tile_cracks = c.take<int>(p.corner_tiles, 64);
  p.tile_base = c.take<int>(p.corner_tiles, 64);
  for (int j = 0; j < 2; ++j) p.tile_n[j] = c.take<int>(p.crack_tiles, 64), p.tile_at[j] = c.take<int>(p.crack_tiles, 64);
  p.next = c.take<int>(m, 64);
  p.leader = c.take<int>(m, 64);
  p.where = c.take<unsigned>(m, 64);
  for (int j = 0; j < 2; ++j) {
    p.jump[j] = c.take<int>(m, 64);
    p.val[j] = c.take<int>(m, 64);
    p.turns[j] = c.take<int>(m, 64);
    p.area[j] = c.take<long long>(m, 64);
  }
  return {true, c.bytes(), p};
}
long label_outlines_workspace_bytes(int h, int w, int max_out, int max_cracks) { return outline_layout(h, w, max_out, max_cracks, nullptr).bytes; }

// ---- the label map around a corner ------------------------------------------------------------------------------------------------

__device__ __forceinline__ int ol_label(const int* __restrict__ label, int max_out, int h, int w, int r, int c) {
  if ((unsigned)r >= (unsigned)h || (unsigned)c >= (unsigned)w) return 0;      // the outside of the image is not k
  const int v = label[(long)r * w + c];
  return v >= 1 && v <= max_out ? v : 0;                    // labels past the capacity are skipped, and not k to the others
}
struct OlCorner {
  int nw, ne, sw, se;
};
__device__ __forceinline__ OlCorner ol_corner(const int* __restrict__ label, int max_out, int h, int w, int x, int y) {
  return {ol_label(label, max_out, h, w, y - 1, x - 1), ol_label(label, max_out, h, w, y - 1, x), ol_label(label, max_out, h, w, y, x - 1),
          ol_label(label, max_out, h, w, y, x)};
}
// bit d: a crack leaves the corner in direction d (0 E: the top of SE, 1 S: the right of SW, 2 W: the bottom of NW, 3 N: the left of NE)
__device__ __forceinline__ int ol_mask(const OlCorner& q) {
  return (int)(q.se > 0 && q.ne != q.se) | (int)(q.sw > 0 && q.se != q.sw) << 1 | (int)(q.nw > 0 && q.sw != q.nw) << 2 |
         (int)(q.ne > 0 && q.nw != q.ne) << 3;
}
__device__ __forceinline__ int ol_corner_mask(const int* __restrict__ label, int max_out, int h, int w, long corner, long corners) {
  if (corner >= corners) return 0;
  const int y = (int)(corner / (w + 1)), x = (int)(corner - (long)y * (w + 1));
  return ol_mask(ol_corner(label, max_out, h, w, x, y));
}

__global__ void ol_init_kernel(OutlinePlanes p, long n_out, long long* __restrict__ out, int* __restrict__ needed) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (long)gridDim.x * blockDim.x) out[i] = 0ll;
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    p.ctl[threadIdx.x] = 0;
    if (threadIdx.x < 4) needed[threadIdx.x] = 0;
  }
}

// ---- census --------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(OL_THREADS) void ol_census_kernel(const int* __restrict__ label, int max_out, int h, int w, OutlinePlanes p) {
  __shared__ int s_w[OL_THREADS / 64];
  const long first = (long)blockIdx.x * OL_TILE + threadIdx.x * OL_ITEMS;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < OL_ITEMS; ++j) mine += __popc(ol_corner_mask(label, max_out, h, w, first + j, p.corners));
  const int total = block_sum<OL_THREADS>(mine, s_w);
  if (threadIdx.x == 0) p.tile_cracks[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void ol_scan_cracks_kernel(OutlinePlanes p, int max_cracks, int* __restrict__ needed) {
  __shared__ int s_w[16];
  const long long total = scan_plane(p.tile_cracks, p.tile_base, p.corner_tiles, s_w);
  if (threadIdx.x == 0) {
    const bool over = total > max_cracks;
    needed[0] = (int)(total > 0x7fffffffll ? 0x7fffffffll : total);
    p.ctl[OL_OVER] = over;
    p.ctl[OL_N] = over ? 0 : (int)total;
  }
}

__global__ __launch_bounds__(OL_THREADS) void ol_base_kernel(const int* __restrict__ label, int max_out, int h, int w, OutlinePlanes p) {
  __shared__ int s_w[OL_THREADS / 64];
  if (p.ctl[OL_OVER]) return;                               // uniform: more cracks than the planes hold
  const long first = (long)blockIdx.x * OL_TILE + threadIdx.x * OL_ITEMS;
  int count[OL_ITEMS], mine = 0;
#pragma unroll
  for (int j = 0; j < OL_ITEMS; ++j) mine += count[j] = __popc(ol_corner_mask(label, max_out, h, w, first + j, p.corners));
  int at = p.tile_base[blockIdx.x] + block_excl_scan<OL_THREADS>(mine, s_w);
#pragma unroll
  for (int j = 0; j < OL_ITEMS; ++j) {
    if (first + j < p.corners) p.base[first + j] = at;
    at += count[j];
  }
}

// ---- successors ------------------------------------------------------------------------------------------------------------------

// rank: the ping-pong set in which the ranks start (the one the leader rounds do not end in)
__global__ __launch_bounds__(OL_THREADS) void ol_successor_kernel(const int* __restrict__ label, int max_out, int h, int w, OutlinePlanes p, int rank) {
  if (p.ctl[OL_OVER]) return;
  const int* __restrict__ base = p.base;
  for (long corner = (long)blockIdx.x * blockDim.x + threadIdx.x; corner < p.corners; corner += (long)gridDim.x * blockDim.x) {
    const int y = (int)(corner / (w + 1)), x = (int)(corner - (long)y * (w + 1));
    const OlCorner q = ol_corner(label, max_out, h, w, x, y);
    const int m = ol_mask(q);
    if (!m) continue;
    const int b = base[corner];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (!((m >> d) & 1)) continue;
      const int i = b + __popc(m & ((1 << d) - 1));
      const int k = d == 0 ? q.se : d == 1 ? q.sw : d == 2 ? q.nw : q.ne;             // the crack's own pixel
      const int hx = x + (d == 0) - (d == 2), hy = y + (d == 1) - (d == 3);
      const OlCorner a = ol_corner(label, max_out, h, w, hx, hy);
      const int ahead_right = d == 0 ? a.se : d == 1 ? a.sw : d == 2 ? a.nw : a.ne;
      const int ahead_left = d == 0 ? a.ne : d == 1 ? a.se : d == 2 ? a.sw : a.nw;
      const int nd = ahead_right != k ? (d + 1) & 3 : ahead_left != k ? d : (d + 3) & 3;
      const int j = base[(long)hy * (w + 1) + hx] + __popc(ol_mask(a) & ((1 << nd) - 1));
      const int turn = nd != d;
      p.next[i] = j;
      p.jump[0][i] = j;
      p.val[0][i] = i;
      p.where[i] = (unsigned)corner << 3 | (unsigned)d << 1 | (unsigned)turn;
      p.turns[rank][i] = turn;
      p.area[rank][i] = (long long)x * hy - (long long)hx * y;
    }
  }
}

// ---- leaders ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(OL_THREADS) void ol_leader_kernel(OutlinePlanes p, int from) {
  const int n = p.ctl[OL_N];
  const int *__restrict__ jin = p.jump[from], *__restrict__ vin = p.val[from];
  int *__restrict__ jout = p.jump[from ^ 1], *__restrict__ vout = p.val[from ^ 1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int j = jin[i];
    vout[i] = min(vin[i], vin[j]);
    jout[i] = jin[j];
  }
}

// lead: the set the leader rounds ended in; the ranks start in the other one
__global__ __launch_bounds__(OL_THREADS) void ol_cut_kernel(OutlinePlanes p, int lead) {
  const int n = p.ctl[OL_N];
  const int *__restrict__ next = p.next, *__restrict__ vin = p.val[lead];
  int *__restrict__ jout = p.jump[lead ^ 1], *__restrict__ vout = p.val[lead ^ 1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int nx = next[i], li = vin[i], ln = vin[nx];
    if (li != ln) p.ctl[OL_LONG] = 1;                       // a cycle longer than the windows: read by later launches only
    p.leader[i] = li;
    jout[i] = ln == nx ? -1 : nx;                           // cut in front of the leader
    vout[i] = 1;
  }
}

// ---- ranks -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(OL_THREADS) void ol_rank_kernel(OutlinePlanes p, int from) {
  if (p.ctl[OL_LONG]) return;
  const int n = p.ctl[OL_N];
  const int *__restrict__ jin = p.jump[from], *__restrict__ vin = p.val[from], *__restrict__ tin = p.turns[from];
  const long long* __restrict__ ain = p.area[from];
  int *__restrict__ jout = p.jump[from ^ 1], *__restrict__ vout = p.val[from ^ 1], *__restrict__ tout = p.turns[from ^ 1];
  long long* __restrict__ aout = p.area[from ^ 1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int j = jin[i];
    int v = vin[i], t = tin[i];
    long long a = ain[i];
    if (j >= 0) v += vin[j], t += tin[j], a += ain[j];
    jout[i] = j >= 0 ? jin[j] : -1;
    vout[i] = v, tout[i] = t, aout[i] = a;
  }
}

// ---- contours --------------------------------------------------------------------------------------------------------------------

// fin: the set the rank rounds ended in.  One workgroup per tile of the crack room; tiles past the cracks count nothing.
__global__ __launch_bounds__(OL_THREADS) void ol_contour_count_kernel(OutlinePlanes p, int fin, int max_len) {
  __shared__ int s_w[2 * OL_THREADS / 64];
  if (p.ctl[OL_OVER] | p.ctl[OL_LONG]) return;              // uniform; both were written by earlier launches
  const int n = p.ctl[OL_N];
  const long first = (long)blockIdx.x * OL_TILE + threadIdx.x * OL_ITEMS;
  int leaders = 0, verts = 0;
#pragma unroll
  for (int j = 0; j < OL_ITEMS; ++j) {
    const long i = first + j;
    if (i < n && p.leader[i] == (int)i) {
      ++leaders;
      verts += p.turns[fin][i];
      if (p.val[fin][i] > max_len) p.ctl[OL_LEN] = 1;       // read by later launches only
    }
  }
  const int mine[2] = {leaders, verts};
  int excl[2], total[2];
  block_excl_scan<OL_THREADS>(mine, excl, total, s_w);
  if (threadIdx.x == 0) p.tile_n[0][blockIdx.x] = total[0], p.tile_n[1][blockIdx.x] = total[1];
}

__global__ __launch_bounds__(1024) void ol_scan_contours_kernel(OutlinePlanes p, int* __restrict__ needed) {
  __shared__ int s_w[16];
  if (p.ctl[OL_OVER]) return;                               // only needed[0] means anything
  if (p.ctl[OL_LONG] | p.ctl[OL_LEN]) {                     // never fragments: no contour, no vertex
    if (threadIdx.x == 0) needed[3] = 1, p.ctl[OL_LONG] = 1;
    return;
  }
  const long long contours = scan_plane(p.tile_n[0], p.tile_at[0], p.crack_tiles, s_w);
  const long long verts = scan_plane(p.tile_n[1], p.tile_at[1], p.crack_tiles, s_w);
  if (threadIdx.x == 0) needed[1] = (int)contours, needed[2] = (int)verts;       // both at most the number of cracks
}

__global__ __launch_bounds__(OL_THREADS) void ol_contours_kernel(const int* __restrict__ label, int max_out, int h, int w, OutlinePlanes p, int fin,
                                                                 long long* __restrict__ out, long long* __restrict__ contours, int max_contours) {
  __shared__ int s_w[2 * OL_THREADS / 64];
  if (p.ctl[OL_OVER] | p.ctl[OL_LONG]) return;
  const int n = p.ctl[OL_N];
  const long first = (long)blockIdx.x * OL_TILE + threadIdx.x * OL_ITEMS;
  if ((long)blockIdx.x * OL_TILE >= n) return;              // uniform
  int nv[OL_ITEMS], leaders = 0, verts = 0;
#pragma unroll
  for (int j = 0; j < OL_ITEMS; ++j) {
    const long i = first + j;
    nv[j] = i < n && p.leader[i] == (int)i ? p.turns[fin][i] : -1;
    if (nv[j] >= 0) ++leaders, verts += nv[j];
  }
  const int mine[2] = {leaders, verts};
  int excl[2], total[2];
  block_excl_scan<OL_THREADS>(mine, excl, total, s_w);
  int c = p.tile_at[0][blockIdx.x] + excl[0], at = p.tile_at[1][blockIdx.x] + excl[1];
  int* __restrict__ first_of = p.jump[fin ^ 1];             // free since the last rank round: a leader's first vertex
#pragma unroll
  for (int j = 0; j < OL_ITEMS; ++j) {
    if (nv[j] < 0) continue;
    const long i = first + j;
    const unsigned wh = p.where[i];
    const int corner = (int)(wh >> 3), d = (int)(wh >> 1) & 3;
    const int y = corner / (w + 1), x = corner - y * (w + 1);
    const int r = y - (d >= 2), col = x - (d == 1 || d == 2);       // the crack's own pixel: E (y, x), S (y, x - 1), W (y - 1, x - 1), N (y - 1, x)
    const int k = label[(long)r * w + col];                 // in 1..max_out: the census saw it
    const long long len = p.val[fin][i], s2 = p.area[fin][i];
    first_of[i] = at;
    if (c < max_contours) {
      long long* row = contours + c;
      const long m = max_contours;
      row[C_LABEL * m] = k, row[C_FIRST * m] = at, row[C_NV * m] = nv[j], row[C_LENGTH * m] = len, row[C_S2 * m] = s2;
    }
    long long* o = out + (k - 1);
    const long rows = max_out;
    atomic_add64(o + O_E * rows, len);
    atomic_add64(o + (s2 > 0 ? O_NO : O_NH) * rows, 1);
    atomic_add64(o + O_NV * rows, nv[j]);
    if (s2 > 0) atomic_add64(o + O_F2 * rows, s2);
    atomic_add64(o + O_S2 * rows, s2);
    ++c, at += nv[j];
  }
}

__global__ __launch_bounds__(OL_THREADS) void ol_vertices_kernel(OutlinePlanes p, int w, int fin, int* __restrict__ vx, int* __restrict__ vy, int max_vertices) {
  if (p.ctl[OL_OVER] | p.ctl[OL_LONG]) return;
  const int n = p.ctl[OL_N];
  const int *__restrict__ turns = p.turns[fin], *__restrict__ first_of = p.jump[fin ^ 1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned wh = p.where[i];
    if (!(wh & 1u)) continue;
    const int s = p.leader[i], nv = turns[s];
    int vi = nv - turns[i] + 1;                             // turns[i] counts this crack's turn: 1..nv
    if (vi == nv) vi = 0;                                   // the last turn is the start's tail
    const long at = (long)first_of[s] + vi;
    if (at >= max_vertices) continue;
    const int corner = (int)(wh >> 3), d = (int)(wh >> 1) & 3;
    const int y = corner / (w + 1), x = corner - y * (w + 1);
    vx[at] = x + (d == 0) - (d == 2);
    vy[at] = y + (d == 1) - (d == 3);
  }
}

int launch_label_outlines(const int* label, int max_out, int h, int w, int max_len, void* workspace, long workspace_bytes, long long* out,
                          long long* contours, int max_contours, int* vx, int* vy, int max_vertices, int max_cracks, int* needed,
                          hipStream_t stream) {
  UNETDC_REQUIRE(label && workspace && needed && (out || max_out == 0) && (contours || max_contours == 0) &&
                     ((vx && vy) || max_vertices == 0),
                 "label_outlines: null pointer");
  const auto lay = outline_layout(h, w, max_out, max_cracks, workspace);
  UNETDC_REQUIRE(lay.ok, "label_outlines: bad geometry (sides 1..16384, h * w < 2^30, non-negative label limit, crack limit 0..2^30)");
  UNETDC_REQUIRE(max_len >= 0 && max_contours >= 0 && max_vertices >= 0, "label_outlines: negative limit (max_len, max_contours, max_vertices)");
  if (int rc = require_workspace("label_outlines", workspace_bytes, lay.bytes)) return rc;
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "label_outlines: workspace must be 8-byte aligned");
  const OutlinePlanes& p = lay.planes;
  int rounds = 0;
  while (rounds < 31 && (1L << rounds) < max_len) ++rounds;
  const int lead = rounds & 1, rank = lead ^ 1, fin = rank ^ (rounds & 1);
  const dim3 block(OL_THREADS);
  const int crack_grid = grid_for(max_cracks, OL_THREADS, OL_MAX_GRID);
  hipLaunchKernelGGL(ol_init_kernel, dim3(grid_for((long)OUTLINE_QUANTITIES * max_out, 256, 1024)), dim3(256), 0, stream, p,
                     (long)OUTLINE_QUANTITIES * max_out, out, needed);
  hipLaunchKernelGGL(ol_census_kernel, dim3(p.corner_tiles), block, 0, stream, label, max_out, h, w, p);
  hipLaunchKernelGGL(ol_scan_cracks_kernel, dim3(1), dim3(1024), 0, stream, p, max_cracks, needed);
  hipLaunchKernelGGL(ol_base_kernel, dim3(p.corner_tiles), block, 0, stream, label, max_out, h, w, p);
  hipLaunchKernelGGL(ol_successor_kernel, dim3(grid_for(p.corners, OL_THREADS, 8192)), block, 0, stream, label, max_out, h, w, p, rank);
  for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(ol_leader_kernel, dim3(crack_grid), block, 0, stream, p, r & 1);
  hipLaunchKernelGGL(ol_cut_kernel, dim3(crack_grid), block, 0, stream, p, lead);
  for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(ol_rank_kernel, dim3(crack_grid), block, 0, stream, p, rank ^ (r & 1));
  if (p.crack_tiles > 0) hipLaunchKernelGGL(ol_contour_count_kernel, dim3(p.crack_tiles), block, 0, stream, p, fin, max_len);
  hipLaunchKernelGGL(ol_scan_contours_kernel, dim3(1), dim3(1024), 0, stream, p, needed);
  if (p.crack_tiles > 0) {
    hipLaunchKernelGGL(ol_contours_kernel, dim3(p.crack_tiles), block, 0, stream, label, max_out, h, w, p, fin, out, contours, max_contours);
    hipLaunchKernelGGL(ol_vertices_kernel, dim3(crack_grid), block, 0, stream, p, w, fin, vx, vy, max_vertices);
  }
  return check_launch("label_outlines kernels");
}

}  // namespace unetdc
