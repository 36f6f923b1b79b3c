// Threshold sweep against an annotation: the confusion matrix of the thresholded mask at EVERY threshold
// of the grid t_k = (float)k / (float)K, k = 0..K-1, from one pass over the output pixels.
//
// The mask rule of ccl.hip (mask_kernel, mask_linear_kernel) is monotone in the threshold: a pixel set at t_k is set at every
// lower one.  So a pixel has one LEVEL, the number of grid thresholds at which it is set, and hist[g][level] (g = annotation
// nonzero) holds every confusion matrix at once: tp_k = sum over level > k of hist[1][level], fp_k likewise from hist[0].
//
//   tap level    lev(p) = #{k : p > t_k}.  For a non-negative, non-NaN float `p > t` is `bits(p) > bits(t)` on the unsigned
//                words, and a negative or NaN p is above no threshold of the grid (t_0 = 0): a guess from p * K, then a walk of
//                at most a few steps along the bit table of the grid in LDS.  The grid is strictly increasing for K <= 1024.
//   nearest      the level of the one source pixel under cv2's index rule (as mask_kernel)
//   linear       the 8-bit bilinear v of mask_linear_kernel changes only where a tap changes: the pixel's level is the largest
//                tap level L with v != 0 when exactly the taps of level >= L are set (four evaluations of the integer formula)
//   histogram    per workgroup [2][K + 1] int32 in LDS; the lanes of a wave that share a bin send ONE add of their number
//                (for_each_wave_key, wave_ops.h: in a micrograph nearly every pixel is background at level 0); the
//                nonzero bins go out as 64-bit integer atomics.  Integers only: the result depends on no order.
#include "kernels.h"
#include "linear_u8.h"
#include "wave_ops.h"

namespace unetdc {

constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_MAX_K = 1024;
constexpr int SWEEP_MAX_GROUPS = 1024;              // every workgroup flushes into the same few words: fewer, longer workgroups
constexpr long SWEEP_MAX_PIXELS = 1L << 40;         // per launch: a workgroup's share stays below 2^31 (int32 LDS bins)

// #{k < K : grid[k] < a} for the bits a of a float in (0, 1); grid[k] = bits of (float)k / (float)K, strictly increasing
__device__ __forceinline__ int sweep_tap_level(unsigned a, const unsigned* grid, int K) {
  if (a == 0u || a > 0x7f800000u) return 0;         // +0, every negative value (sign bit), NaN: above no threshold
  if (a >= 0x3f800000u) return K;                   // >= 1 > t_{K-1}
  int lev = (int)(bits_f32(a) * (float)K);          // within a step or two of the answer; the walks below make it exact
  lev = lev > K ? K : lev;
  while (lev < K && grid[lev] < a) ++lev;
  while (lev > 0 && grid[lev - 1] >= a) --lev;
  return lev;
}

template <bool LINEAR>
__global__ __launch_bounds__(SWEEP_THREADS) void thresh_sweep_kernel(const float* __restrict__ probs, int ph, int pw,
                                                                     const unsigned char* __restrict__ gt, int oh, int ow,
                                                                     long total, double fy, double fx,
                                                                     const int* __restrict__ xofs, const short* __restrict__ xa,
                                                                     const int* __restrict__ yofs, const short* __restrict__ ya,
                                                                     int K, unsigned long long* __restrict__ hist) {
  __shared__ unsigned grid[SWEEP_MAX_K];
  __shared__ int bins[2 * (SWEEP_MAX_K + 1)];
  const int nbins = 2 * (K + 1), lane = threadIdx.x & 63;
  for (int k = threadIdx.x; k < K; k += SWEEP_THREADS) grid[k] = f32_bits((float)k / (float)K);
  for (int b = threadIdx.x; b < nbins; b += SWEEP_THREADS) bins[b] = 0;
  __syncthreads();
  const int npix = oh * ow;                         // sides <= 16384: below 2^31
  const long pstride = (long)ph * pw;
  for (long base = (long)blockIdx.x * SWEEP_THREADS; base < total; base += (long)gridDim.x * SWEEP_THREADS) {
    const long i = base + threadIdx.x;              // the trip count is uniform in a wave: the ballots need all 64 lanes
    const bool live = i < total;
    int bin = -1;
    if (live) {
      const long img = i / npix;
      const int r = (int)(i - img * npix), y = r / ow, x = r - y * ow;
      const float* p = probs + img * pstride;
      int lev;
      if (!LINEAR) {
        int sy = (int)floor(y * fy), sx = (int)floor(x * fx);
        sy = sy < ph - 1 ? sy : ph - 1;
        sx = sx < pw - 1 ? sx : pw - 1;
        lev = sweep_tap_level(f32_bits(p[(long)sy * pw + sx]), grid, K);
      } else {
        const LinearTaps t = linear_u8_taps(xofs, xa, yofs, ya, x, y, pw, ph);
        int l[4];
        l[0] = sweep_tap_level(f32_bits(p[(long)t.sy0 * pw + t.sx0]), grid, K);
        l[1] = sweep_tap_level(f32_bits(p[(long)t.sy0 * pw + t.sx1]), grid, K);
        l[2] = sweep_tap_level(f32_bits(p[(long)t.sy1 * pw + t.sx0]), grid, K);
        l[3] = sweep_tap_level(f32_bits(p[(long)t.sy1 * pw + t.sx1]), grid, K);
        lev = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {               // the mask at threshold l[c] - 1: exactly the taps of level >= l[c] are set
          const int L = l[c];
          const int v = linear_u8_combine(l[0] >= L, l[1] >= L, l[2] >= L, l[3] >= L, t.a0, t.a1, t.b0, t.b1);
          if (v > 0 && L > lev) lev = L;
        }
      }
      bin = (gt[i] != 0 ? K + 1 : 0) + lev;
    }
    for_each_wave_key(bin, live, [&](int lead, int lead_bin, unsigned long long same) {
      if (lane == lead) atomicAdd(&bins[lead_bin], __popcll(same));
    });
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += SWEEP_THREADS) {
    const int c = bins[b];
    if (c) atomicAdd(&hist[b], (unsigned long long)c);
  }
}

static int sweep_groups(long total) {
  const long nb = (total + SWEEP_THREADS - 1) / SWEEP_THREADS;
  return (int)(nb > SWEEP_MAX_GROUPS ? SWEEP_MAX_GROUPS : nb < 1 ? 1 : nb);
}

int launch_thresh_sweep(const float* probs, int n, int ph, int pw, const unsigned char* gt, int oh, int ow, const int* xofs,
                        const short* xcoef, const int* yofs, const short* ycoef, int k, long long* hist, hipStream_t stream) {
  UNETDC_REQUIRE(probs && gt && hist, "thresh_sweep: null pointer");
  UNETDC_REQUIRE(k >= 1 && k <= SWEEP_MAX_K, "thresh_sweep: k = %d outside 1..%d", k, SWEEP_MAX_K);
  UNETDC_REQUIRE(n >= 1 && ph >= 1 && pw >= 1 && oh >= 1 && ow >= 1 && ph <= 16384 && pw <= 16384 && oh <= 16384 && ow <= 16384,
                 "thresh_sweep: bad geometry n=%d %dx%d -> %dx%d (n >= 1, sides 1..16384)", n, ph, pw, oh, ow);
  const bool linear = xofs && xcoef && yofs && ycoef;
  UNETDC_REQUIRE(linear || (!xofs && !xcoef && !yofs && !ycoef), "thresh_sweep: the four resize tables come together or not at all");
  UNETDC_REQUIRE(reinterpret_cast<uintptr_t>(hist) % 8 == 0, "thresh_sweep: hist must be 8-byte aligned");
  const long npix = (long)oh * ow;
  const long per = SWEEP_MAX_PIXELS / npix;          // images per launch (>= 4096)
  for (long first = 0; first < n; first += per) {
    const long m = n - first < per ? n - first : per, total = m * npix;
    const float* p = probs + first * (long)ph * pw;
    const unsigned char* g = gt + first * npix;
    const dim3 grid(sweep_groups(total)), block(SWEEP_THREADS);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(hist);
    if (linear)
      hipLaunchKernelGGL(thresh_sweep_kernel<true>, grid, block, 0, stream, p, ph, pw, g, oh, ow, total, 0.0, 0.0, xofs, xcoef,
                         yofs, ycoef, k, out);
    else
      hipLaunchKernelGGL(thresh_sweep_kernel<false>, grid, block, 0, stream, p, ph, pw, g, oh, ow, total, (double)ph / (double)oh,
                         (double)pw / (double)ow, xofs, xcoef, yofs, ycoef, k, out);
  }
  return check_launch("thresh_sweep_kernel");
}

}  // namespace unetdc
