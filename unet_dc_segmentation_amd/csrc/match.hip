// Sparse contingency table of two int32 label maps: for every pair (a, b) of labels that share a
// pixel, the number of shared pixels, listed in ascending order of (a, b).  Integer atomics only, and the order of the
// output is fixed by a sort on unique keys: two runs give the same bytes.
//
//   match_init_kernel      hash slots empty, counts 0, sort keys at the pad value, the three control words 0
//   match_overlap_kernel   one wave per 64 consecutive pixels of a row, as label_props_kernel.  Only pixels that carry a label
//                          in range on BOTH maps take part.  Lanes with the same (a, b) next to each other form a run (heads
//                          from a ballot of key[x] != key[x - 1]); only the run's head inserts, with the run length as its
//                          count: a few inserts per droplet row, not one per pixel.
//                          Table: open addressing, linear probing, a power of two >= 2 * max_pairs slots.  The 64-bit key
//                          (a << 32) | b is claimed with a compare-and-swap, the count added with a 32-bit atomic add.  Every
//                          claim of an empty slot counts itself; the claim that finds max_pairs claims before it raises the
//                          overflow flag, after which inserts are dropped.  So the table never fills past half (plus the
//                          claims in flight), "overflow" means exactly "more than max_pairs pairs", and a probe sequence
//                          is bounded by the table size: an insert that finds no slot raises the flag and carries on.
//                          Nothing ever waits for another thread.
//   match_compact_kernel   occupied slots -> a dense list, in arrival order (the order is fixed by the sort below)
//   match_sort_*_kernel    bitonic sort of the list by key, padded to a power of two N >= max_pairs with keys above every real
//                          one: strides below 4096 inside LDS (one launch per merge tail), larger strides one launch each.
//                          N log^2 N / 4 compare-exchanges whatever the degrees are: a label that overlaps everything costs
//                          no more than any other table of that capacity.
//   match_emit_kernel      the first min(count, max_pairs) sorted entries -> out_a, out_b, out_n; *out_count
#include "kernels.h"

namespace unetdc {

typedef unsigned long long match_key_t;
constexpr match_key_t MATCH_EMPTY = ~0ull;     // no real key: a and b are positive int32
constexpr int MATCH_SORT_CHUNK = 4096;         // elements one workgroup sorts in LDS (48 KB)
enum { MATCH_CLAIMS = 0, MATCH_OVERFLOW = 1, MATCH_ENTRIES = 2, MATCH_CTL_WORDS = 16 };

struct MatchPlanes {
  int* ctl;            // [MATCH_CTL_WORDS]
  match_key_t* keys;   // [slots]
  int* counts;         // [slots]
  match_key_t* ek;     // [n_sort]
  int* ec;             // [n_sort]
  int slots, n_sort, max_pairs;
};

static long match_pow2_at_least(long v) {
  long p = 1;
  while (p < v) p <<= 1;
  return p;
}

// max_pairs beyond h * w buys nothing: there are at most h * w pairs
static int match_effective_pairs(int h, int w, int max_pairs) {
  const long n = (long)h * w;
  return (long)max_pairs < n ? max_pairs : (int)n;
}

static long match_align64(long v) { return (v + 63) / 64 * 64; }

static MatchPlanes match_planes(void* workspace, int h, int w, int max_pairs) {
  MatchPlanes p;
  p.max_pairs = match_effective_pairs(h, w, max_pairs);
  p.slots = (int)match_pow2_at_least(p.max_pairs > 32 ? 2L * p.max_pairs : 64L);
  p.n_sort = (int)match_pow2_at_least(p.max_pairs > 1 ? p.max_pairs : 1);
  unsigned char* b = reinterpret_cast<unsigned char*>(workspace);
  p.ctl = reinterpret_cast<int*>(b);
  b += match_align64(MATCH_CTL_WORDS * 4);
  p.keys = reinterpret_cast<match_key_t*>(b);
  b += match_align64((long)p.slots * 8);
  p.counts = reinterpret_cast<int*>(b);
  b += match_align64((long)p.slots * 4);
  p.ek = reinterpret_cast<match_key_t*>(b);
  b += match_align64((long)p.n_sort * 8);
  p.ec = reinterpret_cast<int*>(b);
  return p;
}

long label_overlap_workspace_bytes(int h, int w, int max_pairs) {
  const MatchPlanes p = match_planes(nullptr, h, w, max_pairs);
  return match_align64(MATCH_CTL_WORDS * 4) + match_align64((long)p.slots * 8) + match_align64((long)p.slots * 4) +
         match_align64((long)p.n_sort * 8) + match_align64((long)p.n_sort * 4);
}

__global__ void match_init_kernel(MatchPlanes p) {
  const int stride = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = t; i < p.slots; i += stride) {
    p.keys[i] = MATCH_EMPTY;
    p.counts[i] = 0;
  }
  for (int i = t; i < p.n_sort; i += stride) {
    p.ek[i] = MATCH_EMPTY;
    p.ec[i] = 0;
  }
  if (t < MATCH_CTL_WORDS) p.ctl[t] = 0;
}

__device__ __forceinline__ void match_insert(const MatchPlanes& p, match_key_t key, int n) {
  volatile int* overflow = p.ctl + MATCH_OVERFLOW;
  if (*overflow) return;
  const unsigned mask = (unsigned)p.slots - 1u;
  unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
  for (int probe = 0; probe < p.slots; ++probe, slot = (slot + 1u) & mask) {
    match_key_t cur = *reinterpret_cast<volatile match_key_t*>(p.keys + slot);
    if (cur == MATCH_EMPTY) {
      cur = atomicCAS(p.keys + slot, MATCH_EMPTY, key);
      if (cur == MATCH_EMPTY) {                              // this thread claimed the slot: one more pair
        if (atomicAdd(p.ctl + MATCH_CLAIMS, 1) >= p.max_pairs) atomicExch(p.ctl + MATCH_OVERFLOW, 1);
        cur = key;
      }
    }
    if (cur == key) {
      atomicAdd(p.counts + slot, n);
      return;
    }
    if ((probe & 63) == 63 && *overflow) return;
  }
  atomicExch(p.ctl + MATCH_OVERFLOW, 1);                     // no slot: only a table of in-flight claims gets here
}

__global__ __launch_bounds__(256) void match_overlap_kernel(const int* __restrict__ label_a, int max_a,
                                                            const int* __restrict__ label_b, int max_b, int h, int w,
                                                            MatchPlanes p) {
  const int lane = threadIdx.x & 63;
  const int chunks = (w + 63) >> 6;
  const long units = (long)h * chunks;
  const long stride = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += stride) {   // uniform within a wave
    const int y = (int)(u / chunks), x = ((int)(u - (long)y * chunks) << 6) + lane;
    const bool in = x < w;
    const long i = (long)y * w + x;
    const int a = in ? label_a[i] : 0, b = in ? label_b[i] : 0;
    // labels below 1 or above the given maxima take no part
    const match_key_t key = (a > 0 && a <= max_a && b > 0 && b <= max_b) ? ((match_key_t)(unsigned)a << 32) | (unsigned)b : 0ull;
    if (__ballot(key != 0ull) == 0ull) continue;             // wave-uniform: no shared foreground here
    const match_key_t prev = __shfl_up(key, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || key != prev);
    if (key != 0ull && ((heads >> lane) & 1ull)) {
      const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = above ? __ffsll((long long)above) : 64 - lane;     // lanes from this one to the end of its run
      match_insert(p, key, len);
    }
  }
}

__global__ void match_compact_kernel(MatchPlanes p) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.slots; i += gridDim.x * blockDim.x) {
    const match_key_t k = p.keys[i];
    if (k == MATCH_EMPTY) continue;
    const int e = atomicAdd(p.ctl + MATCH_ENTRIES, 1);
    if (e < p.n_sort) {
      p.ek[e] = k;
      p.ec[e] = p.counts[i];
    }
  }
}

// bitonic network: the pair of compare-exchange t at stride j is (l, l + j), ascending where bit k of the index is clear
__device__ __forceinline__ int match_pair_low(int t, int j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// stages k_lo .. k_hi of the network restricted to strides below the chunk: a whole sort of each chunk (k_lo = 2,
// k_hi = chunk) or the tail of one merge stage (k_lo = k_hi = k > chunk)
__global__ __launch_bounds__(1024) void match_sort_local_kernel(match_key_t* __restrict__ ek, int* __restrict__ ec, int n, int k_lo,
                                                                int k_hi) {
  __shared__ match_key_t sk[MATCH_SORT_CHUNK];
  __shared__ int sc[MATCH_SORT_CHUNK];
  const int chunk = n < MATCH_SORT_CHUNK ? n : MATCH_SORT_CHUNK;
  const int base = blockIdx.x * chunk;
  for (int e = threadIdx.x; e < chunk; e += 1024) {
    sk[e] = ek[base + e];
    sc[e] = ec[base + e];
  }
  __syncthreads();
  for (int k = k_lo; k <= k_hi; k <<= 1) {
    for (int j = (k >> 1) < (chunk >> 1) ? (k >> 1) : (chunk >> 1); j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (chunk >> 1); t += 1024) {
        const int l = match_pair_low(t, j), r = l + j;
        const bool ascending = ((base + l) & k) == 0;
        const match_key_t x = sk[l], y = sk[r];
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
    ec[base + e] = sc[e];
  }
}

__global__ void match_sort_global_kernel(match_key_t* __restrict__ ek, int* __restrict__ ec, int n, int j, int k) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < (n >> 1); t += gridDim.x * blockDim.x) {
    const int l = match_pair_low(t, j), r = l + j;
    const bool ascending = (l & k) == 0;
    const match_key_t x = ek[l], y = ek[r];
    if ((x > y) == ascending) {
      const int cx = ec[l], cy = ec[r];
      ek[l] = y, ek[r] = x;
      ec[l] = cy, ec[r] = cx;
    }
  }
}

__global__ void match_emit_kernel(MatchPlanes p, int max_pairs, int* __restrict__ out_count, int* __restrict__ out_a,
                                  int* __restrict__ out_b, int* __restrict__ out_n) {
  const int entries = p.ctl[MATCH_ENTRIES];
  const bool overflow = p.ctl[MATCH_OVERFLOW] != 0 || entries > p.max_pairs;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) *out_count = overflow ? max_pairs + 1 : entries;
  const int m = entries < p.max_pairs ? entries : p.max_pairs;        // p.max_pairs <= max_pairs and <= n_sort
  for (int i = t; i < m; i += gridDim.x * blockDim.x) {
    const match_key_t k = p.ek[i];
    out_a[i] = (int)(k >> 32);
    out_b[i] = (int)(k & 0xffffffffull);
    out_n[i] = p.ec[i];
  }
}

static unsigned match_grid(long items, int per_block, int limit) {
  const long g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : g > limit ? limit : g);
}

int launch_label_overlap(const int* label_a, int max_a, const int* label_b, int max_b, int h, int w, void* workspace,
                         long workspace_bytes, int* out_count, int* out_a, int* out_b, int* out_n, int max_pairs,
                         hipStream_t stream) {
  UNETDC_REQUIRE(label_a && label_b && workspace && out_count && ((out_a && out_b && out_n) || max_pairs == 0),
                 "label_overlap: null pointer");
  UNETDC_REQUIRE(h > 0 && w > 0 && h <= 16384 && w <= 16384 && max_a >= 0 && max_b >= 0 && max_pairs >= 0,
                 "label_overlap: bad geometry (sides 1..16384, non-negative label and pair limits)");
  if (workspace_bytes < label_overlap_workspace_bytes(h, w, max_pairs)) {
    set_error("label_overlap: workspace too small (%ld < %ld bytes)", workspace_bytes, label_overlap_workspace_bytes(h, w, max_pairs));
    return UNETDC_EWORKSPACE;
  }
  const MatchPlanes p = match_planes(workspace, h, w, max_pairs);
  hipLaunchKernelGGL(match_init_kernel, dim3(match_grid(p.slots, 256, 2048)), dim3(256), 0, stream, p);
  const long units = (long)h * ((w + 63) / 64);
  hipLaunchKernelGGL(match_overlap_kernel, dim3(match_grid(units, 4, 8192)), dim3(256), 0, stream, label_a, max_a, label_b, max_b,
                     h, w, p);
  hipLaunchKernelGGL(match_compact_kernel, dim3(match_grid(p.slots, 256, 2048)), dim3(256), 0, stream, p);
  const int n = p.n_sort, chunk = n < MATCH_SORT_CHUNK ? n : MATCH_SORT_CHUNK;
  if (n > 1) {
    hipLaunchKernelGGL(match_sort_local_kernel, dim3(n / chunk), dim3(1024), 0, stream, p.ek, p.ec, n, 2, chunk);
    for (long k = 2L * chunk; k <= n; k <<= 1) {
      for (long j = k >> 1; j >= chunk; j >>= 1)
        hipLaunchKernelGGL(match_sort_global_kernel, dim3(match_grid(n / 2, 256, 4096)), dim3(256), 0, stream, p.ek, p.ec, n, (int)j,
                           (int)k);
      hipLaunchKernelGGL(match_sort_local_kernel, dim3(n / chunk), dim3(1024), 0, stream, p.ek, p.ec, n, (int)k, (int)k);
    }
  }
  hipLaunchKernelGGL(match_emit_kernel, dim3(match_grid(p.max_pairs, 256, 2048)), dim3(256), 0, stream, p, max_pairs, out_count,
                     out_a, out_b, out_n);
  return check_launch("label overlap kernels");
}

}  // namespace unetdc
