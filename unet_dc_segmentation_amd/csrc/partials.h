// Two-stage reductions over partial rows (fixed summation order, no float atomics -> bitwise reproducible): the first-stage
// reducer and the device helpers of the finalisers.  Buffers follow the spare-row contract of kernels.h (SPARE_ROWS).
#pragma once
#include "kernels.h"

namespace unetdc {

// Reduce `nparts` rows of L floats to at most SPARE_ROWS rows written at parts + nparts * L (the caller's spare rows); the
// reduced set comes back through red_ptr / red_rows.  `direct` = row count up to which the consumer reads the rows itself:
// REDUCE_DIRECT for the serial finalisers; the BatchNorm finalisers (256 threads over the rows) save this launch up to _WIDE.
constexpr int REDUCE_DIRECT = 64, REDUCE_DIRECT_WIDE = 512;
int reduce_parts(const float* parts, int nparts, int L, const float** red_ptr, int* red_rows, hipStream_t stream, int direct);

// A workgroup owns FOUR consecutive channels: thread t takes partial rows t, t + 256, ... (one 16-byte load per row and
// statistic -- at most two trips for the <= 512 rows the producers write, all loads in flight at once), fp64 from there
// on: wave shuffle, then the four waves in fixed order through LDS -> deterministic.  (The first form, a serial per-thread
// loop over the rows, cost ~17 us per launch in load latency alone; the second, 32 lanes per channel and 16 dependent trips,
// 6.5-13 us.)
constexpr int FIN_C = 4;

__device__ __forceinline__ double lane32_sum(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}

template <int NROW>
__device__ __forceinline__ void fin_rows(const float* __restrict__ parts, int nparts, int cs, int col, int nch,
                                         double (&acc)[NROW][FIN_C]) {
  const bool vec = nch == FIN_C && ((cs | col) & 3) == 0 && (reinterpret_cast<uintptr_t>(parts) & 15) == 0;
  for (int i = threadIdx.x; i < nparts; i += 256) {
#pragma unroll
    for (int w = 0; w < NROW; ++w) {
      const float* src = parts + ((long)i * NROW + w) * cs + col;
      float v[FIN_C] = {0.f, 0.f, 0.f, 0.f};
      if (vec) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int e = 0; e < FIN_C; ++e) v[e] = t[e];
      } else {
#pragma unroll
        for (int e = 0; e < FIN_C; ++e) if (e < nch) v[e] = src[e];
      }
#pragma unroll
      for (int e = 0; e < FIN_C; ++e) acc[w][e] += (double)v[e];
    }
  }
}

// totals of the workgroup in red[w * FIN_C + e] (valid after the call for every thread)
template <int NROW>
__device__ __forceinline__ void fin_block_sum(double (&acc)[NROW][FIN_C], double* red, double* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < NROW; ++w)
#pragma unroll
    for (int e = 0; e < FIN_C; ++e) {
      double v = acc[w][e];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) red[wave * NROW * FIN_C + w * FIN_C + e] = v;
    }
  __syncthreads();
  if (threadIdx.x < NROW * FIN_C) {
    const int k = threadIdx.x;
    tot[k] = ((red[k] + red[NROW * FIN_C + k]) + red[2 * NROW * FIN_C + k]) + red[3 * NROW * FIN_C + k];
  }
  __syncthreads();
}

}  // namespace unetdc
