// Sparse contingency table of two int32 label maps: for every pair (a, b) of labels that share a
// pixel, the number of shared pixels, listed in ascending order of (a, b).  Integer atomics only, and the order of the
// output is fixed by a sort on unique keys: two runs give the same bytes.
//
// The table, its overflow rule, the compaction, the bitonic sort and the emit are those of pair_table.h (its kernels
// pair_init / pair_compact / pair_sort_* / pair_emit are what used to be match_init / ... here), instantiated with
// addition as the combine step.  This file adds the kernel that fills the table:
//
//   match_overlap_kernel   one wave per 64 consecutive pixels of a row, as label_props_kernel.  Only pixels that carry a label
//                          in range on BOTH maps take part.  Lanes with the same (a, b) next to each other form a run
//                          (wave_runs, wave_ops.h); only the run's head inserts, with the run length as its count: a few
//                          inserts per droplet row, not one per pixel.
#include "pair_table.h"
#include "wave_ops.h"

namespace unetdc {

// the pair table alone.  max_pairs beyond h * w buys nothing: there are at most h * w pairs
static Layout<PairPlanes> match_layout(int h, int w, int max_pairs, void* workspace) {
  if (!(h > 0 && w > 0 && h <= 16384 && w <= 16384 && max_pairs >= 0)) return {false, 0, {}};
  Carver c(workspace);
  const PairPlanes p = pair_carve(c, (int)std::min((long)max_pairs, (long)h * w));
  return {true, c.bytes(), p};
}
long label_overlap_workspace_bytes(int h, int w, int max_pairs) { return match_layout(h, w, max_pairs, nullptr).bytes; }

__global__ __launch_bounds__(256) void match_overlap_kernel(const int* __restrict__ label_a, int max_a,
                                                            const int* __restrict__ label_b, int max_b, int h, int w,
                                                            PairPlanes p) {
  const int lane = threadIdx.x & 63;
  const int chunks = (w + 63) >> 6;
  const long units = (long)h * chunks;
  const long stride = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += stride) {   // uniform within a wave
    const RowUnit px = row_unit(u, chunks, w, lane);
    const int a = px.in ? label_a[px.i] : 0, b = px.in ? label_b[px.i] : 0;
    // labels below 1 or above the given maxima take no part
    const pair_key_t key = (a > 0 && a <= max_a && b > 0 && b <= max_b) ? ((pair_key_t)(unsigned)a << 32) | (unsigned)b : 0ull;
    if (__ballot(key != 0ull) == 0ull) continue;             // wave-uniform: no shared foreground here
    const WaveRuns r = wave_runs(key, lane);
    if (key != 0ull && r.head) pair_insert<PairAdd>(p, key, r.len);
  }
}

int launch_label_overlap(const int* label_a, int max_a, const int* label_b, int max_b, int h, int w, void* workspace,
                         long workspace_bytes, int* out_count, int* out_a, int* out_b, int* out_n, int max_pairs,
                         hipStream_t stream) {
  UNETDC_REQUIRE(label_a && label_b && workspace && out_count && ((out_a && out_b && out_n) || max_pairs == 0),
                 "label_overlap: null pointer");
  const auto lay = match_layout(h, w, max_pairs, workspace);
  UNETDC_REQUIRE(lay.ok && max_a >= 0 && max_b >= 0,
                 "label_overlap: bad geometry (sides 1..16384, non-negative label and pair limits)");
  if (int rc = require_workspace("label_overlap", workspace_bytes, lay.bytes)) return rc;
  const PairPlanes& p = lay.planes;
  pair_table_init<PairAdd>(p, stream);
  const long units = (long)h * ((w + 63) / 64);
  hipLaunchKernelGGL(match_overlap_kernel, dim3(grid_for(units, 4, 8192)), dim3(256), 0, stream, label_a, max_a, label_b, max_b,
                     h, w, p);
  pair_table_list(p, max_pairs, out_count, out_a, out_b, out_n, stream);
  return check_launch("label overlap kernels");
}

}  // namespace unetdc
