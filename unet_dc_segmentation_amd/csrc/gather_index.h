// Index rules shared by the gather kernels of augment.hip, crop.hip and tile.hip, and the ONE per-pixel augmentation body
// (gather_pixel), record checks and launch loop of augment_gather_kernel, crop_gather_kernel and crop_gather_scaled_kernel.
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

// One output pixel (y, x) of an augmented H x W sample, every channel and the mask: the random part of TrainAugment (the
// head of augment.hip) applied to a LATTICE of source pixels.  The three gather kernels differ only in their lattice:
//   L.tap(sy, sx)      a handle on lattice pixel (sy, sx), formed once per tap and used for every channel
//   L.value(handle, c) channel c of that pixel as a float in [0, 1]
//   L.mask(sy, sx)     its mask value as a float
// p: an AugRecord or a CropRecord; oi / om: the addresses of this pixel in channel 0 of the output image and in the output
// mask (channel stride H * W).  The rule and its reasons: the head of augment.hip.
template <class Lattice, class Record>
__device__ __forceinline__ void gather_pixel(const Lattice& L, const Record& p, int C, int H, int W, int y, int x,
                                             const float* __restrict__ fields, float* __restrict__ oi, float* __restrict__ om) {
  const long hw = (long)H * W, pix = (long)y * W + x;
  int sy, sx;
  if (p.field < 0) {
    aug_source(y, x, H, W, p.flags, p.k, sy, sx);
    const auto s = L.tap(sy, sx);
    for (int c = 0; c < C; ++c) oi[c * hw] = aug_bc(L.value(s, c), p);
    *om = L.mask(sy, sx);
    return;
  }
  const float* f = fields + (long)p.field * 2 * hw;
  const float dx = f[pix], dy = f[hw + pix];
  const float fx = floorf(dx), fy = floorf(dy);
  const float tx = dx - fx, ty = dy - fy;                   // exact: the fraction of a float32
  const int ix = x + (int)fx, iy = y + (int)fy;
  decltype(L.tap(0, 0)) s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    aug_source(aug_reflect(iy + (q >> 1), H), aug_reflect(ix + (q & 1), W), H, W, p.flags, p.k, sy, sx);
    s[q] = L.tap(sy, sx);
  }
  const float wx0 = 1.0f - tx, wy0 = 1.0f - ty;
  for (int c = 0; c < C; ++c) {
    const float a00 = aug_bc(L.value(s[0], c), p), a01 = aug_bc(L.value(s[1], c), p);
    const float a10 = aug_bc(L.value(s[2], c), p), a11 = aug_bc(L.value(s[3], c), p);
    oi[c * hw] = wy0 * (wx0 * a00 + tx * a01) + ty * (wx0 * a10 + tx * a11);
  }
  // order 0: the nearest tap, round half up (ties are measure-zero for a smooth float field)
  aug_source(aug_reflect(iy + (ty >= 0.5f), H), aug_reflect(ix + (tx >= 0.5f), W), H, W, p.flags, p.k, sy, sx);
  *om = L.mask(sy, sx);
}

// The checks every gather record shares (who: the entry point's name for the messages, i: the sample)
template <class Record>
inline int check_gather_record(const char* who, int i, const Record& p, const float* fields, int nfields) {
  UNETDC_REQUIRE(p.k >= 0 && p.k <= 3, "%s: sample %d: k = %d (0..3)", who, i, p.k);
  UNETDC_REQUIRE((p.flags & ~(AUG_HFLIP | AUG_VFLIP | AUG_BC)) == 0, "%s: sample %d: bad flags 0x%x", who, i, p.flags);
  UNETDC_REQUIRE(p.field >= -1 && p.field < nfields, "%s: sample %d: field slot %d outside [-1, %d)", who, i, p.field, nfields);
  UNETDC_REQUIRE(p.field < 0 || fields, "%s: sample %d draws elastic but fields is null", who, i);
  return UNETDC_OK;
}

// Records go BY VALUE in the launch arguments, AUG_MAX_BATCH per launch: launch(batch, m, n0) once per batch of m records
// that starts at sample n0.  Batch: a struct of one array r[AUG_MAX_BATCH] of records; the slots past m are zero.
template <class Batch, class Record, class Launch>
inline void for_gather_batches(const Record* params, int n, Launch launch) {
  for (int n0 = 0; n0 < n; n0 += AUG_MAX_BATCH) {
    const int m = n - n0 < AUG_MAX_BATCH ? n - n0 : AUG_MAX_BATCH;
    Batch b = {};
    for (int i = 0; i < m; ++i) b.r[i] = params[n0 + i];
    launch(b, m, n0);
  }
}

}  // namespace unetdc
