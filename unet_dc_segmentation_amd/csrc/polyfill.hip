// Polygons -> int32 label map: exact even-odd fill at pixel centres (the rule is stated once in
// utils/polygon_masks.py).  Vertices are int32 sub-pixel coordinates (256 per pixel); pixel (r, c) has its centre at
// (256 c + 128, 256 r + 128).  An edge ordered so that y0 < y1 crosses row r iff y0 <= Y_r < y1, and then toggles the parity of
// its polygon from column k = floor(((Y_r - y0)(x1 - x0) + (x0 - 128)(y1 - y0)) / (256 (y1 - y0))) + 1 on.  A pixel gets the
// largest label among the polygons that contain its centre.
//
//   fill_kernel<int>    the output plane: zeros (wave_ops.h, as scan_plane and for_each_wave_key below)
//   pf_items_kernel     one wave per polygon: the rows whose centre line its edges can cross and the columns a toggle can start at, both
//                       clipped to the image (its box), and the number of those rows.  An item is (polygon, row)
//   pf_scan_kernel      one workgroup: exclusive scan of the rows per polygon, the item bases; the total behind them
//   pf_fill_kernel      one wave per item, PF_WAVES items per workgroup and trip: the polygon by binary search in the bases;
//                       lanes stride over the edges of every ring, a crossing edge XORs one bit of the row's bit mask in LDS
//                       (one 64-bit division per crossing); prefix XOR inside every 64-bit word by shifts, across words by a
//                       ballot; an atomic maximum of the label at every set bit
//   pf_census_kernel    pixels per label value 1..n, one atomic add per wave and distinct value
//   pf_relabel_kernel   a lookup old -> new, in place
// Every dependent step is its own launch; nothing waits on another workgroup.  Integer atomic maxima and adds only: bitwise
// reproducible.  The boxes and bases are made here, from the vertices, never taken from the caller: every index the fill
// kernel forms lies inside the box, and the ranges it reads from the caller's index arrays are clamped to the vertex list.
#include <climits>

#include "kernels.h"
#include "wave_ops.h"
#include "workspace.h"

namespace unetdc {

constexpr int PF_THREADS = 256, PF_WAVES = PF_THREADS / 64;
constexpr int PF_MAX_GRID = 2048;                 // workgroups of the fill kernel: PF_MAX_GRID * PF_WAVES items per trip
constexpr int PF_WORDS = 16384 / 64;              // 64-bit words of a row's bit mask: a box is at most 16384 columns wide
constexpr int PF_MAX_POLYS = 1 << 22, PF_MAX_VERTS = 1 << 24;

struct PolyfillPlanes {
  int4* box;          // [P] r0, r1, c0, c1: rows r0 .. r1 - 1, columns c0 .. c1 - 1
  int* rows;          // [P] items of the polygon
  int* base;          // [P + 1] exclusive scan of rows; base[P] = items
};

static Layout<PolyfillPlanes> polyfill_layout(int h, int w, int n_polys, int n_rings, int n_verts, void* workspace) {
  if (!(h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30) && n_polys >= 0 && n_polys <= PF_MAX_POLYS &&
        n_verts >= 0 && n_verts <= PF_MAX_VERTS && n_rings >= 0 && (long)n_rings * 3 <= n_verts && n_polys <= n_rings &&
        (long)n_polys * h < (1L << 31)))                      // items <= P * h: the bound the host can check
    return {false, 0, {}};
  Carver c(workspace);
  PolyfillPlanes p;
  p.box = c.take<int4>(n_polys, 64);
  p.rows = c.take<int>(n_polys, 64);
  p.base = c.take<int>((long)n_polys + 1, 64);
  return {true, c.bytes(), p};
}
long polygon_fill_workspace_bytes(int h, int w, int n_polys, int n_rings, int n_verts) {
  const auto lay = polyfill_layout(h, w, n_polys, n_rings, n_verts, nullptr);
  return lay.ok ? lay.bytes : -1;
}

__device__ __forceinline__ int pf_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void pf_items_kernel(const int2* __restrict__ verts, const int* __restrict__ ring_first,
                                                        const int* __restrict__ poly_first_ring, const int* __restrict__ poly_label,
                                                        int n_polys, int n_rings, int n_verts, int h, int w, PolyfillPlanes p) {
  // one wave per polygon: the lanes stride over its vertices (one coalesced read), then a butterfly over the four extremes
  const int lane = threadIdx.x & 63, waves = (gridDim.x * blockDim.x) >> 6;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n_polys; i += waves) {
    const int ra = pf_clamp(poly_first_ring[i], 0, n_rings), rb = pf_clamp(poly_first_ring[i + 1], ra, n_rings);
    const int a = pf_clamp(ring_first[ra], 0, n_verts), b = pf_clamp(ring_first[rb], a, n_verts);
    int xmin = INT_MAX, xmax = INT_MIN, ymin = INT_MAX, ymax = INT_MIN;
    for (int v = a + lane; v < b; v += 64) {
      const int2 q = verts[v];
      xmin = min(xmin, q.x), xmax = max(xmax, q.x), ymin = min(ymin, q.y), ymax = max(ymax, q.y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      xmin = min(xmin, __shfl_xor(xmin, o, 64)), xmax = max(xmax, __shfl_xor(xmax, o, 64));
      ymin = min(ymin, __shfl_xor(ymin, o, 64)), ymax = max(ymax, __shfl_xor(ymax, o, 64));
    }
    int4 box = {0, 0, 0, 0};                                // every lane holds the extremes; lane 0 writes
    if (b > a && poly_label[i] > 0) {
      // Y_r = 256 r + 128 in [ymin, ymax): r from ceil((ymin - 128) / 256) to ceil((ymax - 128) / 256) - 1; a toggle column is
      // floor((x - 128) / 256) + 1 for a crossing at x in [xmin, xmax].  64-bit: the caller's coordinates are not trusted
      const long r0 = ((long)ymin - 128 + 255) >> 8, r1 = ((long)ymax - 128 + 255) >> 8;
      const long c0 = (((long)xmin - 128) >> 8) + 1, c1 = (((long)xmax - 128) >> 8) + 1;
      box.x = (int)min(max(r0, 0L), (long)h), box.y = (int)min(max(r1, 0L), (long)h);
      box.z = (int)min(max(c0, 0L), (long)w), box.w = (int)min(max(c1, 0L), (long)w);
    }
    if (lane == 0) {
      p.box[i] = box;
      p.rows[i] = box.w > box.z ? max(box.y - box.x, 0) : 0;
    }
  }
}

// One workgroup of 1024: exclusive scan of rows[0 .. n) into base[0 .. n); base[n] = the total (< 2^31: the layout refuses
// n * h beyond that).
__global__ __launch_bounds__(1024) void pf_scan_kernel(PolyfillPlanes p, int n) {
  __shared__ int s_w[16];
  const long long total = scan_plane(p.rows, p.base, n, s_w);
  if (threadIdx.x == 0) p.base[n] = (int)total;
}

__global__ __launch_bounds__(PF_THREADS) void pf_fill_kernel(const int2* __restrict__ verts, const int* __restrict__ ring_first,
                                                             const int* __restrict__ poly_first_ring, const int* __restrict__ poly_label,
                                                             int n_polys, int n_rings, int n_verts, int w, PolyfillPlanes p,
                                                             int* __restrict__ out) {
  __shared__ unsigned long long s_bits[PF_WAVES][PF_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* bits = s_bits[wave];
  unsigned* bits32 = reinterpret_cast<unsigned*>(bits);
  const int* __restrict__ base = p.base;
  const int n_items = base[n_polys];
  // the trip count is the same for the waves of a workgroup: every wave reaches every barrier, with or without an item
  for (long first = (long)blockIdx.x * PF_WAVES; first < n_items; first += (long)gridDim.x * PF_WAVES) {
    const long item = first + wave;
    const bool live = item < n_items;
    int poly = 0, r = 0, c0 = 0, span = 0, label = 0;
    if (live) {
      int lo = 0, hi = n_polys;                             // base[lo] <= item < base[hi]: base[0] = 0, base[n_polys] = n_items
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] > (int)item) hi = mid; else lo = mid;
      }
      poly = lo;                                            // base[lo] <= item < base[lo + 1]: a polygon with rows
      const int4 box = p.box[poly];
      r = box.x + ((int)item - base[poly]);
      c0 = box.z, span = box.w - box.z;                     // 1 .. 16384
      label = poly_label[poly];
    }
    const int words = (span + 63) >> 6;
    for (int j = lane; j < words; j += 64) bits[j] = 0ull;
    __syncthreads();
    if (live) {
      const long Y = 256L * r + 128;
      const int ra = pf_clamp(poly_first_ring[poly], 0, n_rings), rb = pf_clamp(poly_first_ring[poly + 1], ra, n_rings);
      for (int ring = ra; ring < rb; ++ring) {
        const int a = pf_clamp(ring_first[ring], 0, n_verts), b = pf_clamp(ring_first[ring + 1], a, n_verts);
        for (int v = a + lane; v < b; v += 64) {
          int2 q0 = verts[v], q1 = verts[v + 1 < b ? v + 1 : a];
          if ((q0.y <= Y) == (q1.y <= Y)) continue;         // horizontal edges never count
          if (q0.y > q1.y) {
            const int2 t = q0;
            q0 = q1, q1 = t;
          }
          const long dy = (long)q1.y - q0.y;                // > 0
          const long num = (Y - q0.y) * ((long)q1.x - q0.x) + ((long)q0.x - 128) * dy, den = 256 * dy;
          long k = num / den;
          if (num % den < 0) --k;                           // floor
          k += 1 - c0;
          if (k >= span) continue;                          // toggles nothing inside the box
          const int at = k < 0 ? 0 : (int)k;                // left of the image: the whole row from column 0
          atomicXor(&bits32[at >> 5], 1u << (at & 31));
        }
      }
    }
    __syncthreads();
    unsigned carry = 0;                                     // parity of the words before this trip's
    for (int j0 = 0; j0 < words; j0 += 64) {                // uniform in the wave
      const int j = j0 + lane;
      unsigned long long x = j < words ? bits[j] : 0ull;
      x ^= x << 1, x ^= x << 2, x ^= x << 4, x ^= x << 8, x ^= x << 16, x ^= x << 32;
      const unsigned long long tops = __ballot((x >> 63) != 0);
      const unsigned before = (__popcll(tops & ((1ull << lane) - 1)) & 1) ^ carry;
      if (before) x = ~x;
      if (j < words) bits[j] = x;
      carry ^= __popcll(tops) & 1;
    }
    __syncthreads();
    if (live) {
      int* __restrict__ row = out + (long)r * w + c0;
      for (int c = lane; c < span; c += 64)
        if ((bits32[c >> 5] >> (c & 31)) & 1u) atomicMax(&row[c], label);
    }
    __syncthreads();
  }
}

// The lanes of a wave hold consecutive pixels, mostly of one or two labels: one add per distinct value and wave.
__global__ __launch_bounds__(256) void pf_census_kernel(const int* __restrict__ label, long n, int n_labels, long long* __restrict__ area) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long trips = (n + stride - 1) / stride;             // uniform: every lane of a wave makes every trip
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long t = 0; t < trips; ++t, i += stride) {
    const int v = i < n ? label[i] : 0;
    for_each_wave_key(v, v >= 1 && v <= n_labels, [&](int lead, int lv, unsigned long long same) {
      if ((threadIdx.x & 63) == lead) atomic_add64(area + (lv - 1), __popcll(same));
    });
  }
}

__global__ __launch_bounds__(256) void pf_relabel_kernel(int* __restrict__ label, long n, const int* __restrict__ lut, int n_lut) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int v = label[i];
    if (v >= 1 && v <= n_lut) label[i] = lut[v - 1];
  }
}

int launch_polygon_fill(const int* verts, const int* ring_first, const int* poly_first_ring, const int* poly_label, int n_polys,
                        int n_rings, int n_verts, int h, int w, int* labels_out, void* workspace, long workspace_bytes,
                        hipStream_t stream) {
  const auto lay = polyfill_layout(h, w, n_polys, n_rings, n_verts, workspace);
  UNETDC_REQUIRE(lay.ok, "polygon_fill: bad geometry (sides 1..16384, h * w < 2^30, polygons 0..2^22 and at most the rings, "
                         "rings at most vertices / 3, vertices 0..2^24, polygons * h < 2^31)");
  UNETDC_REQUIRE(labels_out && workspace && ring_first && poly_first_ring && (n_polys == 0 || (verts && poly_label)),
                 "polygon_fill: null pointer");
  if (int rc = require_workspace("polygon_fill", workspace_bytes, lay.bytes)) return rc;
  UNETDC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "polygon_fill: workspace must be 16-byte aligned");
  const PolyfillPlanes& p = lay.planes;
  const long n = (long)h * w;
  launch_fill(labels_out, n, 0, grid_for(n, 256 * 4, 4096), stream);
  if (n_polys > 0) {
    const int2* v2 = reinterpret_cast<const int2*>(verts);
    hipLaunchKernelGGL(pf_items_kernel, dim3(grid_for(n_polys, 256 / 64, 4096)), dim3(256), 0, stream, v2, ring_first, poly_first_ring, poly_label,
                       n_polys, n_rings, n_verts, h, w, p);
    hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(1024), 0, stream, p, n_polys);
    hipLaunchKernelGGL(pf_fill_kernel, dim3(grid_for((long)n_polys * h, PF_WAVES, PF_MAX_GRID)), dim3(PF_THREADS), 0, stream, v2, ring_first,
                       poly_first_ring, poly_label, n_polys, n_rings, n_verts, w, p, labels_out);
  }
  return check_launch("polygon_fill kernels");
}

static bool pf_plane_ok(int h, int w) { return h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30); }

int launch_label_census(const int* label, int h, int w, int n_labels, long long* area, hipStream_t stream) {
  UNETDC_REQUIRE(pf_plane_ok(h, w) && n_labels >= 0, "label_census: bad geometry (sides 1..16384, h * w < 2^30, a non-negative label limit)");
  UNETDC_REQUIRE(label && (area || n_labels == 0), "label_census: null pointer");
  if (n_labels == 0) return UNETDC_OK;
  const long n = (long)h * w;
  launch_fill(area, (long)n_labels, 0ll, grid_for(n_labels, 256, 1024), stream);
  hipLaunchKernelGGL(pf_census_kernel, dim3(grid_for(n, 256 * 4, 4096)), dim3(256), 0, stream, label, n, n_labels, area);
  return check_launch("label_census kernels");
}

int launch_label_relabel(int* label, int h, int w, const int* lut, int n_lut, hipStream_t stream) {
  UNETDC_REQUIRE(pf_plane_ok(h, w) && n_lut >= 0, "label_relabel: bad geometry (sides 1..16384, h * w < 2^30, a non-negative table length)");
  UNETDC_REQUIRE(label && (lut || n_lut == 0), "label_relabel: null pointer");
  if (n_lut == 0) return UNETDC_OK;
  const long n = (long)h * w;
  hipLaunchKernelGGL(pf_relabel_kernel, dim3(grid_for(n, 256 * 4, 4096)), dim3(256), 0, stream, label, n, lut, n_lut);
  return check_launch("label_relabel kernel");
}

}  // namespace unetdc
