// Index rules and the per-tap brightness / contrast step shared by the gather kernels of augment.hip, crop.hip and tile.hip.
#pragma once
#include "kernels.h"

namespace unetdc {

// reflect-101 of any int coordinate into 0..dim-1 (period 2 (dim - 1), dim == 1 -> 0): utils/tiling.py:fold
__device__ __forceinline__ int tile_fold(int i, int dim) {
  if ((unsigned)i < (unsigned)dim) return i;
  if (dim == 1) return 0;
  const int p = 2 * (dim - 1);
  int m = i % p;
  m = m < 0 ? m + p : m;
  return m < dim ? m : p - m;
}

// scipy.ndimage mode "reflect" (half-sample symmetric, period 2n) applied to an integer tap index
__device__ inline int aug_reflect(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  m = m < 0 ? m + p : m;
  return m < n ? m : p - 1 - m;
}

// (y, x) in the flipped + rotated image -> (sy, sx) in the source image (H x W; H == W whenever k is odd)
__device__ inline void aug_source(int y, int x, int H, int W, int flags, int k, int& sy, int& sx) {
  int fy = y, fx = x;
  if (k == 1) { fy = x; fx = W - 1 - y; }
  else if (k == 2) { fy = H - 1 - y; fx = W - 1 - x; }
  else if (k == 3) { fy = H - 1 - x; fx = y; }
  sy = (flags & AUG_VFLIP) ? H - 1 - fy : fy;
  sx = (flags & AUG_HFLIP) ? W - 1 - fx : fx;
}

// The inverse of aug_source: (sy, sx) in the source image -> (y, x) in the flipped + rotated image
__device__ inline void aug_dest(int sy, int sx, int H, int W, int flags, int k, int& y, int& x) {
  const int fy = (flags & AUG_VFLIP) ? H - 1 - sy : sy;
  const int fx = (flags & AUG_HFLIP) ? W - 1 - sx : sx;
  y = fy; x = fx;
  if (k == 1) { y = W - 1 - fx; x = fy; }
  else if (k == 2) { y = H - 1 - fy; x = W - 1 - fx; }
  else if (k == 3) { y = fx; x = H - 1 - fy; }
}

// p: an AugRecord or a CropRecord (flags, alpha, beta_max)
template <class Record>
__device__ inline float aug_bc(float v, const Record& p) {
  if (!(p.flags & AUG_BC)) return v;
  // two roundings, as numpy's float32 steps.  __fmul_rn / __fadd_rn are plain operators in HIP, which the backend fuses into
  // one FMA under -ffp-contract=fast (1-ulp differences from numpy); the empty asm makes the product opaque to that fusion
  float m = __fmul_rn(p.alpha, v);
  asm volatile("" : "+v"(m));
  const float t = __fadd_rn(m, p.beta_max);
  return fminf(fmaxf(t, 0.0f), 1.0f);
}

}  // namespace unetdc
