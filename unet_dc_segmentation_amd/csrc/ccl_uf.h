// Lock-free union-find on an int parent array, shared by ccl.hip (4-connected components) and split.hip (basin merging).
#pragma once
#include "common.h"

namespace unetdc {

// parent pointers only ever decrease and every value ever stored in L[x] is an ancestor of x in the final forest, so a
// stale read costs extra hops, never correctness; the agent-scope relaxed loads read through to L2 anyway, where the
// atomicMin of the merges executes
__device__ __forceinline__ int ccl_find(const int* L, int x) {
  int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) { x = p; p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  return x;
}

__device__ __forceinline__ void ccl_unite(int* L, int a, int b) {
  for (;;) {
    a = ccl_find(L, a);
    b = ccl_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }           // a < b: hang the larger root under the smaller
    const int old = atomicMin(&L[b], a);
    if (old == b) return;                                   // b was still a root: done
    b = old;                                                // somebody re-parented b meanwhile: continue from there
  }
}

}  // namespace unetdc
