// Lock-free table of label pairs with one int32 value each, and its deterministic listing: shared by match.hip (the value is
// a pixel count, combined by addition) and neighbors.hip (the value is a squared distance, combined by minimum).
//
//   pair_init_kernel       hash slots empty, values at the combine step's neutral element, sort keys at the pad value, the
//                          control words 0
//   pair_insert<Combine>   Table: open addressing, linear probing, a power of two >= 2 * max_pairs slots.  The 64-bit key
//                          (a << 32) | b is claimed with a compare-and-swap, the value combined with a 32-bit atomic.  Every
//                          claim of an empty slot counts itself; the claim that finds max_pairs claims before it raises the
//                          overflow flag, after which inserts are dropped.  So the table never fills past half (plus the
//                          claims in flight), "overflow" means exactly "more than max_pairs pairs", and a probe sequence
//                          is bounded by the table size: an insert that finds no slot raises the flag and carries on.
//                          Nothing ever waits for another thread.
//   pair_compact_kernel    occupied slots -> a dense list, in arrival order (the order is fixed by the sort below)
//   pair_sort_*_kernel     bitonic sort of the list by key, padded to a power of two N >= max_pairs with keys above every real
//                          one: strides below 4096 inside LDS (one launch per merge tail), larger strides one launch each.
//                          N log^2 N / 4 compare-exchanges whatever the degrees are: a label that is paired with everything
//                          costs no more than any other table of that capacity.  The launches are those of the capacity (the
//                          host does not know the count); the kernels read the count and run the network of the power of two
//                          that holds the entries, so a short list in a roomy table costs empty launches, not a full sort.
//   pair_emit_kernel       the first min(count, max_pairs) sorted entries -> out_a, out_b, out_v; *out_count
//
// The kernels are static: each translation unit that includes this header carries its own copies.
#pragma once
#include "kernels.h"

namespace unetdc {

typedef unsigned long long pair_key_t;
constexpr pair_key_t PAIR_EMPTY = ~0ull;      // no real key: a and b are positive int32
constexpr int PAIR_SORT_CHUNK = 4096;         // elements one workgroup sorts in LDS (48 KB)
// the words from PAIR_USER on belong to the table's owner; pair_init_kernel zeroes them too
enum { PAIR_CLAIMS = 0, PAIR_OVERFLOW = 1, PAIR_ENTRIES = 2, PAIR_USER = 3, PAIR_CTL_WORDS = 16 };

struct PairPlanes {
  int* ctl;           // [PAIR_CTL_WORDS]
  pair_key_t* keys;   // [slots]
  int* vals;          // [slots]
  pair_key_t* ek;     // [n_sort]
  int* ev;            // [n_sort]
  int slots, n_sort, max_pairs;
};

// the combine step of an insert, and the value an untouched slot holds
struct PairAdd {
  static constexpr int NEUTRAL = 0;
  static __device__ __forceinline__ void combine(int* slot, int v) { atomicAdd(slot, v); }
};
struct PairMin {
  static constexpr int NEUTRAL = 0x7fffffff;
  static __device__ __forceinline__ void combine(int* slot, int v) {
    if (v < *reinterpret_cast<volatile int*>(slot)) atomicMin(slot, v);   // the value only ever falls: a stale read costs an atomic
  }
};

static long pair_pow2_at_least(long v) {
  long p = 1;
  while (p < v) p <<= 1;
  return p;
}

// the table's five planes, each rounded to 64 bytes; the owner carves its own planes behind them.
// max_pairs: already cut to what the caller's problem can hold
static PairPlanes pair_carve(Carver& c, int max_pairs) {
  PairPlanes p;
  p.max_pairs = max_pairs;
  p.slots = (int)pair_pow2_at_least(p.max_pairs > 32 ? 2L * p.max_pairs : 64L);
  p.n_sort = (int)pair_pow2_at_least(p.max_pairs > 1 ? p.max_pairs : 1);
  p.ctl = c.take<int>(PAIR_CTL_WORDS, 64);
  p.keys = c.take<pair_key_t>(p.slots, 64);
  p.vals = c.take<int>(p.slots, 64);
  p.ek = c.take<pair_key_t>(p.n_sort, 64);
  p.ev = c.take<int>(p.n_sort, 64);
  return p;
}

static __global__ void pair_init_kernel(PairPlanes p, int neutral) {
  const int stride = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = t; i < p.slots; i += stride) {
    p.keys[i] = PAIR_EMPTY;
    p.vals[i] = neutral;
  }
  for (int i = t; i < p.n_sort; i += stride) {
    p.ek[i] = PAIR_EMPTY;
    p.ev[i] = 0;
  }
  if (t < PAIR_CTL_WORDS) p.ctl[t] = 0;
}

template <typename Combine>
__device__ __forceinline__ void pair_insert(const PairPlanes& p, pair_key_t key, int v) {
  volatile int* overflow = p.ctl + PAIR_OVERFLOW;
  if (*overflow) return;
  const unsigned mask = (unsigned)p.slots - 1u;
  unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
  for (int probe = 0; probe < p.slots; ++probe, slot = (slot + 1u) & mask) {
    pair_key_t cur = *reinterpret_cast<volatile pair_key_t*>(p.keys + slot);
    if (cur == PAIR_EMPTY) {
      cur = atomicCAS(p.keys + slot, PAIR_EMPTY, key);
      if (cur == PAIR_EMPTY) {                              // this thread claimed the slot: one more pair
        if (atomicAdd(p.ctl + PAIR_CLAIMS, 1) >= p.max_pairs) atomicExch(p.ctl + PAIR_OVERFLOW, 1);
        cur = key;
      }
    }
    if (cur == key) {
      Combine::combine(p.vals + slot, v);
      return;
    }
    if ((probe & 63) == 63 && *overflow) return;
  }
  atomicExch(p.ctl + PAIR_OVERFLOW, 1);                     // no slot: only a table of in-flight claims gets here
}

static __global__ void pair_compact_kernel(PairPlanes p) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.slots; i += gridDim.x * blockDim.x) {
    const pair_key_t k = p.keys[i];
    if (k == PAIR_EMPTY) continue;
    const int e = atomicAdd(p.ctl + PAIR_ENTRIES, 1);
    if (e < p.n_sort) {
      p.ek[e] = k;
      p.ev[e] = p.vals[i];
    }
  }
}

// bitonic network: the pair of compare-exchange t at stride j is (l, l + j), ascending where bit k of the index is clear
__device__ __forceinline__ int pair_sort_low(int t, int j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// the network's size for this list: the power of two that holds the compacted entries, at most n_sort.  Behind it lie pad
// keys only, which are where a sort of the whole plane would leave them
static __device__ __forceinline__ int pair_sort_size(const int* ctl, int n_sort) {
  const int e = ctl[PAIR_ENTRIES];
  if (e >= n_sort) return n_sort;
  int n = 1;
  while (n < e) n <<= 1;
  return n;
}

// stages k_lo .. k_hi of the network restricted to strides below the chunk: a whole sort of each chunk (k_lo = 2,
// k_hi = chunk) or the tail of one merge stage (k_lo = k_hi = k > chunk); launched for the capacity n_sort, run for the list
static __global__ __launch_bounds__(1024) void pair_sort_local_kernel(const int* __restrict__ ctl, pair_key_t* __restrict__ ek,
                                                                      int* __restrict__ ev, int n_sort, int k_lo, int k_hi) {
  __shared__ pair_key_t sk[PAIR_SORT_CHUNK];
  __shared__ int sc[PAIR_SORT_CHUNK];
  const int n = pair_sort_size(ctl, n_sort);
  const int chunk = n < PAIR_SORT_CHUNK ? n : PAIR_SORT_CHUNK;
  const int base = blockIdx.x * chunk;
  if (base >= n || k_lo > n) return;                        // the whole block: no barrier has been reached
  if (k_hi > n) k_hi = n;
  for (int e = threadIdx.x; e < chunk; e += 1024) {
    sk[e] = ek[base + e];
    sc[e] = ev[base + e];
  }
  __syncthreads();
  for (int k = k_lo; k <= k_hi; k <<= 1) {
    for (int j = (k >> 1) < (chunk >> 1) ? (k >> 1) : (chunk >> 1); j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (chunk >> 1); t += 1024) {
        const int l = pair_sort_low(t, j), r = l + j;
        const bool ascending = ((base + l) & k) == 0;
        const pair_key_t x = sk[l], y = sk[r];
        if ((x > y) == ascending) {
          const int cx = sc[l], cy = sc[r];
          sk[l] = y, sk[r] = x;
          sc[l] = cy, sc[r] = cx;
        }
      }
      __syncthreads();
    }
  }
  for (int e = threadIdx.x; e < chunk; e += 1024) {
    ek[base + e] = sk[e];
    ev[base + e] = sc[e];
  }
}

static __global__ void pair_sort_global_kernel(const int* __restrict__ ctl, pair_key_t* __restrict__ ek, int* __restrict__ ev,
                                               int n_sort, int j, int k) {
  const int n = pair_sort_size(ctl, n_sort);
  if (k > n) return;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < (n >> 1); t += gridDim.x * blockDim.x) {
    const int l = pair_sort_low(t, j), r = l + j;
    const bool ascending = (l & k) == 0;
    const pair_key_t x = ek[l], y = ek[r];
    if ((x > y) == ascending) {
      const int cx = ev[l], cy = ev[r];
      ek[l] = y, ek[r] = x;
      ev[l] = cy, ev[r] = cx;
    }
  }
}

static __global__ void pair_emit_kernel(PairPlanes p, int max_pairs, int* __restrict__ out_count, int* __restrict__ out_a,
                                        int* __restrict__ out_b, int* __restrict__ out_v) {
  const int entries = p.ctl[PAIR_ENTRIES];
  const bool overflow = p.ctl[PAIR_OVERFLOW] != 0 || entries > p.max_pairs;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) *out_count = overflow ? max_pairs + 1 : entries;
  const int m = entries < p.max_pairs ? entries : p.max_pairs;        // p.max_pairs <= max_pairs and <= n_sort
  for (int i = t; i < m; i += gridDim.x * blockDim.x) {
    const pair_key_t k = p.ek[i];
    out_a[i] = (int)(k >> 32);
    out_b[i] = (int)(k & 0xffffffffull);
    out_v[i] = p.ev[i];
  }
}

template <typename Combine>
static void pair_table_init(const PairPlanes& p, hipStream_t stream) {
  hipLaunchKernelGGL(pair_init_kernel, dim3(grid_for(p.slots, 256, 2048)), dim3(256), 0, stream, p, Combine::NEUTRAL);
}

// the filled table -> the sorted list in ek / ev (the first min(entries, max_pairs) of it in the outputs) and *out_count
static void pair_table_list(const PairPlanes& p, int max_pairs, int* out_count, int* out_a, int* out_b, int* out_v,
                            hipStream_t stream) {
  hipLaunchKernelGGL(pair_compact_kernel, dim3(grid_for(p.slots, 256, 2048)), dim3(256), 0, stream, p);
  const int n = p.n_sort, chunk = n < PAIR_SORT_CHUNK ? n : PAIR_SORT_CHUNK;
  if (n > 1) {
    hipLaunchKernelGGL(pair_sort_local_kernel, dim3(n / chunk), dim3(1024), 0, stream, p.ctl, p.ek, p.ev, n, 2, chunk);
    for (long k = 2L * chunk; k <= n; k <<= 1) {
      for (long j = k >> 1; j >= chunk; j >>= 1)
        hipLaunchKernelGGL(pair_sort_global_kernel, dim3(grid_for(n / 2, 256, 4096)), dim3(256), 0, stream, p.ctl, p.ek, p.ev, n, (int)j,
                           (int)k);
      hipLaunchKernelGGL(pair_sort_local_kernel, dim3(n / chunk), dim3(1024), 0, stream, p.ctl, p.ek, p.ev, n, (int)k, (int)k);
    }
  }
  hipLaunchKernelGGL(pair_emit_kernel, dim3(grid_for(p.max_pairs, 256, 2048)), dim3(256), 0, stream, p, max_pairs, out_count,
                     out_a, out_b, out_v);
}

}  // namespace unetdc
