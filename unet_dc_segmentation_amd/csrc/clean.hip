// Mask cleaning between the threshold and every droplet stage: hysteresis thresholding and hole
// filling of a {0,1} mask, both as 4-connected component problems on the lock-free union-find of ccl_uf.h.
//
//   hysteresis   union-find over the pixels of W; every pixel with S = W = 1 sets a flag at its root; M = the pixels of W
//                whose root carries the flag
//   holes        union-find over the BACKGROUND of M; per root the pixel count (integer atomic add) and, in bit 30 of the
//                same word, "a pixel of this class lies on the first / last row / column" (atomic or); a background pixel is
//                filled when its root has no border bit and its area is within the limit
//   counts       {pixels of M not in S, holes filled, pixels filled, holes left open}: one integer atomic add per wave
//
// Every kernel is a grid-stride loop over pixels whose trip count is uniform within a wave (the ballots and shuffles below
// need all 64 lanes).  Flags that several threads set to the same value, integer atomics and the shared union-find only:
// the result depends on no order.  Workspace: L[n], aux[n] (int32 each), 4 count words.
#include "kernels.h"
#include "ccl_uf.h"
#include "wave_ops.h"

namespace unetdc {

constexpr int CLEAN_BORDER = 1 << 30;               // aux[root]: bit 30 = touches the image border, bits 0..29 = area (n < 2^30)
constexpr int CLEAN_THREADS = 256;

struct CleanPlanes {
  int *L, *aux, *counts;
};

// L[i] = i, aux[i] = 0; the first launch of a call also clears the four counts
__global__ void clean_init_kernel(int* __restrict__ L, int* __restrict__ aux, int n, int* __restrict__ zero_counts) {
  if (zero_counts && blockIdx.x == 0 && threadIdx.x < 4) zero_counts[threadIdx.x] = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    L[i] = i;
    aux[i] = 0;
  }
}

// 4-connectivity over the pixels with (mask != 0) == FG: right and down neighbours
template <bool FG>
__global__ void clean_merge_kernel(const unsigned char* __restrict__ mask, int* __restrict__ L, int h, int w) {
  const int n = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if ((mask[i] != 0) != FG) continue;
    const int y = i / w, x = i - y * w;
    if (x + 1 < w && (mask[i + 1] != 0) == FG) ccl_unite(L, i, i + 1);
    if (y + 1 < h && (mask[i + w] != 0) == FG) ccl_unite(L, i, i + w);
  }
}

// seed[root] = 1 for every pixel that is both strong and weak (all writers store the same value)
__global__ void clean_seed_kernel(const unsigned char* __restrict__ strong, const unsigned char* __restrict__ weak,
                                  const int* __restrict__ L, int* __restrict__ seed, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (strong[i] && weak[i]) seed[ccl_find(L, i)] = 1;
}

// out[i] = W[i] and the class of i is seeded; counts[0] += pixels selected that are not strong.  out may be strong or weak
// itself: a thread reads only its own pixel of either before it writes that pixel.
__global__ __launch_bounds__(CLEAN_THREADS) void clean_select_kernel(const unsigned char* strong, const unsigned char* weak,
                                                                     const int* __restrict__ L, const int* __restrict__ seed,
                                                                     unsigned char* out, int n, int* __restrict__ counts) {
  int added = 0;
  for (int base = blockIdx.x * CLEAN_THREADS; base < n; base += gridDim.x * CLEAN_THREADS) {
    const int i = base + threadIdx.x;
    if (i >= n) continue;
    const bool s = strong[i] != 0;
    const bool m = weak[i] != 0 && seed[ccl_find(L, i)] != 0;
    out[i] = m ? 1 : 0;
    added += m && !s;
  }
  added = wave_sum(added);
  if ((threadIdx.x & 63) == 0 && added) atomicAdd(&counts[0], added);
}

// per background class: area and border bit at the root; L compressed to the root.  The lanes of a wave that share a root
// (nearly always all of them: 64 consecutive pixels of the outside, or of one hole) send ONE add of their number.
__global__ __launch_bounds__(CLEAN_THREADS) void clean_area_kernel(const unsigned char* __restrict__ mask, int* __restrict__ L,
                                                                   int* __restrict__ aux, int h, int w) {
  const int n = h * w, lane = threadIdx.x & 63;
  for (int base = blockIdx.x * CLEAN_THREADS; base < n; base += gridDim.x * CLEAN_THREADS) {
    const int i = base + threadIdx.x;
    const bool bg = i < n && mask[i] == 0;
    int r = -1;
    bool border = false;
    if (bg) {
      r = ccl_find(L, i);
      L[i] = r;                                             // a root keeps L[r] = r
      const int y = i / w, x = i - y * w;
      border = y == 0 || y == h - 1 || x == 0 || x == w - 1;
    }
    for_each_wave_key(r, bg, [&](int lead, int r0, unsigned long long same) {
      const unsigned long long edge = __ballot(bg && r == r0 && border);
      if (lane == lead) {
        atomicAdd(&aux[r0], __popcll(same));
        if (edge) atomicOr(&aux[r0], CLEAN_BORDER);
      }
    });
  }
}

// out[i] = M[i], or 1 where i is background of a class without border bit whose area is within the limit (limit < 0: any);
// counts[1..3] += holes filled, pixels filled, holes left open (a hole is counted at its root pixel).  out may be mask itself.
__global__ __launch_bounds__(CLEAN_THREADS) void clean_fill_kernel(const unsigned char* mask, const int* __restrict__ L,
                                                                   const int* __restrict__ aux, int limit, unsigned char* out,
                                                                   int n, int* __restrict__ counts) {
  int holes = 0, pixels = 0, open = 0;
  for (int base = blockIdx.x * CLEAN_THREADS; base < n; base += gridDim.x * CLEAN_THREADS) {
    const int i = base + threadIdx.x;
    if (i >= n) continue;
    unsigned char v = mask[i] != 0;
    if (!v) {
      const int r = L[i], a = aux[r];                       // compressed by clean_area_kernel
      if (!(a & CLEAN_BORDER)) {
        if (limit < 0 || a <= limit) {
          v = 1;
          ++pixels;
          holes += r == i;
        } else {
          open += r == i;
        }
      }
    }
    out[i] = v;
  }
  holes = wave_sum(holes);
  pixels = wave_sum(pixels);
  open = wave_sum(open);
  if ((threadIdx.x & 63) == 0) {
    if (holes) atomicAdd(&counts[1], holes);
    if (pixels) atomicAdd(&counts[2], pixels);
    if (open) atomicAdd(&counts[3], open);
  }
}

// weak == NULL and max_hole_area == 0: the bytes of strong as they are
__global__ void clean_copy_kernel(const unsigned char* in, unsigned char* out, int n, int* __restrict__ counts) {
  if (blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = 0;
  if (in == out) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = in[i];
}

// L, aux, then the four count words in a 64-byte block
static Layout<CleanPlanes> clean_layout(int h, int w, void* workspace) {
  if (!(h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30))) return {false, 0, {}};
  Carver c(workspace);
  CleanPlanes p;
  p.L = c.take<int>((long)h * w);
  p.aux = c.take<int>((long)h * w);
  p.counts = c.take<int>(4, 64);
  return {true, c.bytes(), p};
}
long mask_clean_workspace_bytes(int h, int w) { return clean_layout(h, w, nullptr).bytes; }

// [a, a + na) and [b, b + nb) share a byte
static bool clean_overlap(const void* a, long na, const void* b, long nb) {
  const char *p = static_cast<const char*>(a), *q = static_cast<const char*>(b);
  return p && q && p < q + nb && q < p + na;
}

int launch_mask_clean(const unsigned char* strong, const unsigned char* weak, int h, int w, int max_hole_area, void* workspace,
                      long workspace_bytes, unsigned char* out_mask, int* out_counts, hipStream_t stream) {
  UNETDC_REQUIRE(strong && workspace && out_mask, "mask_clean: null pointer");
  const auto lay = clean_layout(h, w, workspace);
  UNETDC_REQUIRE(lay.ok, "mask_clean: bad geometry (sides 1..16384)");
  // a short workspace is UNETDC_EINVAL here, not UNETDC_EWORKSPACE (include/unetdc_hip.h)
  if (int rc = require_workspace("mask_clean", workspace_bytes, lay.bytes, UNETDC_EINVAL)) return rc;
  UNETDC_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0 && reinterpret_cast<uintptr_t>(out_counts) % 4 == 0,
                 "mask_clean: workspace and out_counts must be 4-byte aligned");
  const int n = h * w;
  UNETDC_REQUIRE((out_mask == strong || !clean_overlap(out_mask, n, strong, n)) &&
                     (out_mask == weak || !clean_overlap(out_mask, n, weak, n)),
                 "mask_clean: out_mask may be strong or weak itself, but not overlap either partly");
  UNETDC_REQUIRE(!clean_overlap(workspace, lay.bytes, out_mask, n) && !clean_overlap(workspace, lay.bytes, strong, n) &&
                     !clean_overlap(workspace, lay.bytes, weak, n) && !clean_overlap(workspace, lay.bytes, out_counts, 16) &&
                     !clean_overlap(out_counts, 16, out_mask, n) && !clean_overlap(out_counts, 16, strong, n) &&
                     !clean_overlap(out_counts, 16, weak, n),
                 "mask_clean: the workspace and out_counts may overlap nothing else");
  CleanPlanes p = lay.planes;
  if (out_counts) p.counts = out_counts;
  const dim3 grid(grid_for(n, CLEAN_THREADS, 4096)), block(CLEAN_THREADS);
  if (!weak && max_hole_area == 0) {
    hipLaunchKernelGGL(clean_copy_kernel, grid, block, 0, stream, strong, out_mask, n, p.counts);
    return check_launch("clean_copy_kernel");
  }
  const unsigned char* m = strong;                          // the mask the hole stage reads
  if (weak) {
    hipLaunchKernelGGL(clean_init_kernel, grid, block, 0, stream, p.L, p.aux, n, p.counts);
    hipLaunchKernelGGL(clean_merge_kernel<true>, grid, block, 0, stream, weak, p.L, h, w);
    hipLaunchKernelGGL(clean_seed_kernel, grid, block, 0, stream, strong, weak, p.L, p.aux, n);
    hipLaunchKernelGGL(clean_select_kernel, grid, block, 0, stream, strong, weak, p.L, p.aux, out_mask, n, p.counts);
    m = out_mask;
  }
  if (max_hole_area != 0) {
    hipLaunchKernelGGL(clean_init_kernel, grid, block, 0, stream, p.L, p.aux, n, weak ? nullptr : p.counts);
    hipLaunchKernelGGL(clean_merge_kernel<false>, grid, block, 0, stream, m, p.L, h, w);
    hipLaunchKernelGGL(clean_area_kernel, grid, block, 0, stream, m, p.L, p.aux, h, w);
    hipLaunchKernelGGL(clean_fill_kernel, grid, block, 0, stream, m, p.L, p.aux, max_hole_area, out_mask, n, p.counts);
  }
  return check_launch("clean kernels");
}

}  // namespace unetdc
