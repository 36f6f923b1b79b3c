// The wave64 idioms of the image-side kernels, each stated once ("wave idioms of the image-side kernels").
// Device-only and inlined: nothing here launches, allocates or keeps state.  Two preconditions hold throughout:
//   ALL LANES   every function that ballots or shuffles is called by all 64 lanes of the wave together: from straight-line
//               code, or from a loop or branch whose condition is uniform in the wave.  A lane without work passes
//               live = false (or a key of 0); it does not skip the call.
//   ALL WAVES   the block_* functions and scan_plane hold barriers: every thread of the workgroup calls them, the same number
//               of times.
#pragma once
#include "common.h"

namespace unetdc {

// the 64-bit integer add of the result tables (HIP has the unsigned overload only; two's complement makes it the signed one)
__device__ __forceinline__ void atomic_add64(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// inclusive prefix sum over the lanes: lane l gets v[0] + .. + v[l]
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// ---- runs of equal keys ---------------------------------------------------------------------------------------------------------
// Lanes that hold the same key next to each other form a run; lane 0 always starts one.  A run is reduced inside the wave and
// only its head lane issues atomics.
struct WaveRuns {
  unsigned long long heads;   // bit l: lane l starts a run
  int len;                    // lanes from this one to the end of its run (1..64)
  int tail;                   // the last lane of this lane's run
  bool head;                  // this lane starts a run
};
template <typename K>
__device__ __forceinline__ WaveRuns wave_runs(K key, int lane) {
  const K prev = __shfl_up(key, 1, 64);
  WaveRuns r;
  r.heads = __ballot(lane == 0 || key != prev);
  // the run of this lane ends one lane before the next head above it
  const unsigned long long above = lane == 63 ? 0ull : r.heads >> (lane + 1);
  r.len = above ? __ffsll((long long)above) : 64 - lane;
  r.tail = lane + r.len - 1;
  r.head = (r.heads >> lane) & 1ull;
  return r;
}
// the lanes from this one to the end of its run, as a ballot mask (a shift by 64 is undefined: one run over the whole wave)
__device__ __forceinline__ unsigned long long run_mask(const WaveRuns& r, int lane) {
  return (r.len == 64 ? ~0ull : (1ull << r.len) - 1ull) << lane;
}
// Segmented suffix reduction: after the step o a lane holds op over the lanes from itself to the end of its run or to
// lane + 2 o - 1; at the end a head holds its whole run.  A lane takes its partner's value only when the partner lies in its run.
template <typename T, typename Op>
__device__ __forceinline__ T run_reduce(T v, const WaveRuns& r, int lane, Op op) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_down(v, o, 64);
    if (lane + o <= r.tail) v = op(v, up);
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T run_sum(T v, const WaveRuns& r, int lane) {
  return run_reduce(v, r, lane, [](T a, T b) { return a + b; });
}
template <typename T>
__device__ __forceinline__ T run_min(T v, const WaveRuns& r, int lane) {
  return run_reduce(v, r, lane, [](T a, T b) { return min(a, b); });
}
template <typename T>
__device__ __forceinline__ T run_max(T v, const WaveRuns& r, int lane) {
  return run_reduce(v, r, lane, [](T a, T b) { return max(a, b); });
}

// One trip per distinct key among the live lanes, wherever they sit in the wave: fn(lead, key, same) with the first lane that
// holds the key, the key, and the ballot of the live lanes that hold it.  All lanes run fn, so it may ballot and shuffle; the
// one atomic per key belongs under `if (lane == lead)`.  The trip count comes from ballots: uniform in the wave.
template <typename K, typename F>
__device__ __forceinline__ void for_each_wave_key(K key, bool live, F fn) {
  unsigned long long todo = __ballot(live);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const K lead_key = __shfl(key, lead, 64);
    const unsigned long long same = __ballot(live && key == lead_key);
    fn(lead, lead_key, same);
    todo &= ~same;
  }
}

// ---- one wave per 64 consecutive pixels of a row ----------------------------------------------------------------------------------
// A map of width w has chunks = (w + 63) >> 6 units per row; unit u is uniform in the wave, so the loop over units is too.
struct RowUnit {
  int y, x;
  bool in;      // x < w: the last chunk of a row may be ragged
  long i;       // y * w + x
};
__device__ __forceinline__ RowUnit row_unit(long u, int chunks, int w, int lane) {
  const int y = (int)(u / chunks), x = ((int)(u - (long)y * chunks) << 6) + lane;
  return {y, x, x < w, (long)y * w + x};
}

// ---- the workgroup ------------------------------------------------------------------------------------------------------------
// Sum of v over the workgroup, returned to every thread.  lds: THREADS / 64 words; a barrier lies between two calls on the same lds.
template <int THREADS>
__device__ __forceinline__ int block_sum(int v, int* lds) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int u = 0; u < THREADS / 64; ++u) s += lds[u];
  return s;
}

// Exclusive scan of N quantities at once over the THREADS threads of a workgroup, in thread order, and the totals: a wave scan,
// then the wave totals through LDS.  lds: N * THREADS / 64 words, free again on return.
template <int THREADS, int N>
__device__ __forceinline__ void block_excl_scan(const int (&v)[N], int (&excl)[N], int (&total)[N], int* lds) {
  constexpr int WAVES = THREADS / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl[N];
#pragma unroll
  for (int q = 0; q < N; ++q) incl[q] = wave_incl_scan(v[q], lane);
  if (lane == 63) {
#pragma unroll
    for (int q = 0; q < N; ++q) lds[q * WAVES + wave] = incl[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    excl[q] = incl[q] - v[q], total[q] = 0;
#pragma unroll
    for (int u = 0; u < WAVES; ++u) {
      const int t = lds[q * WAVES + u];
      excl[q] += u < wave ? t : 0;
      total[q] += t;
    }
  }
  __syncthreads();
}
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int* lds) {      // one quantity, no total
  const int in[1] = {v};
  int excl[1], total[1];
  block_excl_scan<THREADS, 1>(in, excl, total, lds);
  return excl[0];
}

// ONE workgroup of THREADS: exclusive scan of in[0 .. n) into out[0 .. n), THREADS entries a trip, in index order; returns the
// 64-bit total to every thread.  A prefix past 2^31 is cut: nothing reads the scan then.  out may be in itself, or in - 1
// (the inclusive scan in place): a trip reads its entries before its first barrier and writes behind it, and no trip reads what
// an earlier one wrote.  lds: THREADS / 64 words.
template <int THREADS = 1024>
__device__ __forceinline__ long long scan_plane(const int* in, int* out, int n, int* lds) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  long long run = 0;
  for (int base = 0; base < n; base += THREADS) {
    const int i = base + t, v = i < n ? in[i] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    long long before = 0, tile = 0;
#pragma unroll
    for (int u = 0; u < THREADS / 64; ++u) {
      const int q = lds[u];
      before += u < wave ? q : 0;
      tile += q;
    }
    if (i < n) out[i] = (int)(run + before + incl - v);
    run += tile;
    __syncthreads();
  }
  return run;
}

// ---- fill ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void fill_kernel(T* __restrict__ a, long n, T v) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) a[i] = v;
}
template <typename T>
inline void launch_fill(T* a, long n, T v, int groups, hipStream_t stream) {
  hipLaunchKernelGGL(fill_kernel<T>, dim3(groups), dim3(256), 0, stream, a, n, v);
}

}  // namespace unetdc
