// OpenCV's 8-bit INTER_LINEAR, stated once for the kernels that resize with it: resize_linear_chw_kernel (preprocess.hip),
// mask_linear_kernel (ccl.hip), the LINEAR branch of thresh_sweep_kernel (sweep.hip) and crop_scaled_value (crop.hip).
#pragma once
#include "common.h"

namespace unetdc {

// One output value from its four source values and the 11-bit coefficient pairs (a0, a1) along x, (b0, b1) along y: the
// horizontal pass r = p0 * a0 + p1 * a1 per row, then the vertical pass with its >>4 / >>16 / +2 >>2 roundings.  Not clamped:
// every caller clamps and stores in its own type.
__device__ __forceinline__ int linear_u8_combine(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
  const int r0 = p00 * a0 + p01 * a1, r1 = p10 * a0 + p11 * a1;
  return (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
}

// The taps of destination pixel (dy, dx) from the host tables (utils/data_loader.py:linear_tables): xofs / yofs hold the
// source index of the first tap, xa / ya the two coefficients per destination index.  The second x tap stops at W - 1, both
// y taps are clamped to 0..H-1 (the per-axis border rule of that function).  For mask_linear_kernel and thresh_sweep_kernel;
// resize_linear_chw_kernel writes the same look-up out, for the reason given there.
struct LinearTaps {
  int sx0, sx1, sy0, sy1, a0, a1, b0, b1;
};
__device__ __forceinline__ LinearTaps linear_u8_taps(const int* __restrict__ xofs, const short* __restrict__ xa,
                                                     const int* __restrict__ yofs, const short* __restrict__ ya, int dx, int dy,
                                                     int W, int H) {
  LinearTaps t;
  t.sx0 = xofs[dx];
  t.sx1 = min(t.sx0 + 1, W - 1);
  const int sy = yofs[dy];
  t.sy0 = min(max(sy, 0), H - 1);
  t.sy1 = min(max(sy + 1, 0), H - 1);
  t.a0 = xa[2 * dx]; t.a1 = xa[2 * dx + 1]; t.b0 = ya[2 * dy]; t.b1 = ya[2 * dy + 1];
  return t;
}

}  // namespace unetdc
