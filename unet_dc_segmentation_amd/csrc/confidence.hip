// Per-droplet confidence and test-time-augmentation disagreement from an int32 label map and the probability map it came from
// (the rule is stated once in utils/droplet_confidence.py).  Every per-pixel quantity is an integer: the
// probability quantised to 16 bits, q = rint(clamp(p, 0, 1) * 65535) with the product in fp32; its binary entropy from a
// 65536-entry uint16 table (no logarithm here); the flag |q - q(thresh)| <= q(band); with an envelope (lo, hi: the per-pixel
// minimum and maximum over the variants) spread = q(hi) - q(lo) and the flag !(lo > thresh) && hi > thresh.  Sums, counts,
// minima and maxima are accumulated with integer atomics only: the result does not depend on the order in which anything runs.
//
//   label_confidence_init     sums and counts 0, minima INT64_MAX, maxima -1 on out[CONF_QUANTITIES][max_out]; out_image zeros
//   label_confidence_kernel   the frame of label_props_kernel (shape.hip): one wave per 64 consecutive pixels of a row, runs of
//                             equal labels (row_unit and wave_runs, wave_ops.h), only a run's head lane issues atomics.
//                               sums, minima, maxima   run_sum / run_min / run_max; q^2 reaches 2^32 per pixel, so its
//                                                      partials are 64-bit; 64 * 65535 fits 32 bits
//                               counts                 one ballot per flag, popcount under the run's lane mask
//                             A wave without a droplet pixel skips all of that.  The image totals stay in registers over the
//                             grid-stride loop -- the counts as wave-uniform popcounts of ballots, the three sums per lane --
//                             and are reduced once at its end: across the wave, then over the workgroup's four waves in LDS,
//                             one atomic per workgroup and quantity.  The grid is capped at 2048 workgroups so that a wave
//                             of a 1040 x 1388 map walks about three chunks per reduction.
//                             The probability is read at the nearest-neighbour source pixel of unetdc_mask_from_probs: the row
//                             index is wave-uniform, the column index one fp64 product per lane.  At the identity geometry the
//                             load is coalesced; a 512 x 512 plane is 1 MB and stays in L2 while the rows of a 1040 x 1388
//                             label map walk over it.  The table is 128 KB.
#include "kernels.h"
#include "wave_ops.h"

namespace unetdc {

enum { C_N = 0, C_SQ, C_SQQ, C_MINQ, C_MAXQ, C_NBAND, C_SH, C_SSPREAD, C_MAXSPREAD, C_NUNSTABLE };
enum { CI_NPX = 0, CI_NFG, CI_SHALL, CI_SHFG, CI_NBANDALL, CI_NBANDFG, CI_NUNSTABLEALL, CI_SSPREADALL };
static_assert(C_NUNSTABLE + 1 == CONF_QUANTITIES && CI_SSPREADALL + 1 == CONF_IMAGE_QUANTITIES, "confidence quantities");

constexpr long long CONF_MIN_INIT = 0x7fffffffffffffffll;
constexpr int CONF_WAVES = 4, CONF_MAX_GROUPS = 2048;

__global__ void label_confidence_init_kernel(long long* __restrict__ out, int max_out, long long* __restrict__ out_image) {
  const long n = (long)CONF_QUANTITIES * max_out;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n + CONF_IMAGE_QUANTITIES; i += (long)gridDim.x * blockDim.x) {
    if (i < n) {
      const int q = (int)(i / max_out);
      out[i] = q == C_MINQ ? CONF_MIN_INIT : (q == C_MAXQ || q == C_MAXSPREAD) ? -1ll : 0ll;
    } else {
      out_image[i - n] = 0ll;
    }
  }
}

// 0..65535; a NaN gives 0 (fmaxf returns the other operand)
__device__ __forceinline__ int conf_quant(float p) {
  const int q = __float2int_rn(__fmul_rn(fminf(fmaxf(p, 0.f), 1.f), 65535.f));
  return min(max(q, 0), 65535);
}

__global__ __launch_bounds__(64 * CONF_WAVES) void label_confidence_kernel(
    const int* __restrict__ label, int max_out, int h, int w, const float* __restrict__ probs, const float* __restrict__ plo,
    const float* __restrict__ phi, int ph, int pw, double fy, double fx, float thresh, float band,
    const unsigned short* __restrict__ table, long long* __restrict__ out, long long* __restrict__ out_image,
    unsigned char* __restrict__ out_entropy, unsigned char* __restrict__ out_spread) {
  __shared__ long long totals[CONF_WAVES][CONF_IMAGE_QUANTITIES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (w + 63) >> 6;
  const long units = (long)h * chunks;
  const long stride = (long)gridDim.x * CONF_WAVES;
  const int qt = conf_quant(thresh), bq = conf_quant(band);
  const bool env = plo != nullptr;                           // uniform
  long long t_px = 0, t_fg = 0, t_ball = 0, t_bfg = 0, t_uall = 0;      // wave-uniform counts
  long long t_hall = 0, t_hfg = 0, t_sall = 0;                          // per-lane sums, reduced across the wave after the loop
  for (long u = (long)blockIdx.x * CONF_WAVES + wave; u < units; u += stride) {        // uniform within a wave
    const auto [y, x, in, i] = row_unit(u, chunks, w, lane);
    const int kraw = in ? label[i] : 0;
    const bool fg = kraw > 0;                                // foreground whatever max_out
    const int k = (kraw < 0 || kraw > max_out) ? 0 : kraw;   // labels past the capacity are skipped, never written
    int sy = (int)floor(y * fy), sx = (int)floor(x * fx);
    sy = sy < ph - 1 ? sy : ph - 1;
    sx = sx < pw - 1 ? sx : pw - 1;
    const long si = (long)sy * pw + sx;
    int q = 0, hq = 0, spread = 0;
    bool inband = false, unstable = false;
    if (in) {
      q = conf_quant(probs[si]);
      hq = (int)table[q];
      const int d = q - qt;
      inband = (d < 0 ? -d : d) <= bq;
      if (env) {
        const float lo = plo[si], hi = phi[si];
        spread = conf_quant(hi) - conf_quant(lo);
        unstable = !(lo > thresh) && hi > thresh;
      }
      if (out_entropy) out_entropy[i] = (unsigned char)(hq >> 8);
      if (out_spread) out_spread[i] = (unsigned char)(spread >> 8);
    }
    const unsigned long long m_fg = __ballot(fg), m_band = __ballot(inband), m_un = __ballot(unstable);
    t_px += __popcll(__ballot(in));
    t_fg += __popcll(m_fg);
    t_hall += hq;
    t_hfg += fg ? hq : 0;
    t_ball += __popcll(m_band);
    t_bfg += __popcll(m_band & m_fg);
    t_uall += __popcll(m_un);
    t_sall += spread;
    if (__ballot(k > 0) == 0ull) continue;                   // wave-uniform: no droplet pixel here
    const WaveRuns runs = wave_runs(k, lane);
    const int sq = run_sum(q, runs, lane), qmin = run_min(q, runs, lane), qmax = run_max(q, runs, lane);
    const int sh = run_sum(hq, runs, lane);
    const long long sqq = run_sum((long long)q * q, runs, lane);
    int ss = spread, smax = spread;
    if (env) ss = run_sum(spread, runs, lane), smax = run_max(spread, runs, lane);
    if (k > 0 && runs.head) {
      const unsigned long long run = run_mask(runs, lane);
      long long* o = out + (k - 1);
      const long r = max_out;
      atomic_add64(o + C_N * r, runs.len);
      atomic_add64(o + C_SQ * r, sq);
      atomic_add64(o + C_SQQ * r, sqq);
      atomicMin(o + C_MINQ * r, (long long)qmin);
      atomicMax(o + C_MAXQ * r, (long long)qmax);
      const int nb = __popcll(m_band & run);
      if (nb) atomic_add64(o + C_NBAND * r, nb);
      atomic_add64(o + C_SH * r, sh);
      if (env) {
        atomic_add64(o + C_SSPREAD * r, ss);
        atomicMax(o + C_MAXSPREAD * r, (long long)smax);
        const int nu = __popcll(m_un & run);
        if (nu) atomic_add64(o + C_NUNSTABLE * r, nu);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    t_hall += __shfl_down(t_hall, o, 64);
    t_hfg += __shfl_down(t_hfg, o, 64);
    t_sall += __shfl_down(t_sall, o, 64);
  }
  if (lane == 0) {
    long long* t = totals[wave];
    t[CI_NPX] = t_px, t[CI_NFG] = t_fg, t[CI_SHALL] = t_hall, t[CI_SHFG] = t_hfg;
    t[CI_NBANDALL] = t_ball, t[CI_NBANDFG] = t_bfg, t[CI_NUNSTABLEALL] = t_uall, t[CI_SSPREADALL] = t_sall;
  }
  __syncthreads();
  if (threadIdx.x < CONF_IMAGE_QUANTITIES) {
    long long v = 0;
#pragma unroll
    for (int j = 0; j < CONF_WAVES; ++j) v += totals[j][threadIdx.x];
    if (v) atomic_add64(out_image + threadIdx.x, v);
  }
}

int launch_label_confidence(const int* label, int max_out, int h, int w, const float* probs, const float* lo, const float* hi,
                            int ph, int pw, float thresh, float band, const unsigned short* table, long long* out,
                            long long* out_image, unsigned char* out_entropy, unsigned char* out_spread, hipStream_t stream) {
  UNETDC_REQUIRE(label && probs && table && out_image && (out || max_out == 0), "label_confidence: null pointer");
  UNETDC_REQUIRE((lo == nullptr) == (hi == nullptr), "label_confidence: the envelope is both lo and hi, or neither");
  UNETDC_REQUIRE(!out_spread || lo, "label_confidence: the spread map needs an envelope");
  UNETDC_REQUIRE(h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30) && max_out >= 0 && ph > 0 && pw > 0,
                 "label_confidence: bad geometry (sides 1..16384)");
  UNETDC_REQUIRE(band >= 0.f && band <= 0.5f, "label_confidence: the band must lie in 0..0.5");
  const long ni = ((long)CONF_QUANTITIES * max_out + CONF_IMAGE_QUANTITIES + 255) / 256;
  hipLaunchKernelGGL(label_confidence_init_kernel, dim3((unsigned)(ni > 1024 ? 1024 : ni)), dim3(256), 0, stream, out, max_out,
                     out_image);
  const long nb = ((long)h * ((w + 63) / 64) + CONF_WAVES - 1) / CONF_WAVES;
  // cv2's nearest index rule in double precision, as launch_mask_from_probs states it
  hipLaunchKernelGGL(label_confidence_kernel, dim3((unsigned)(nb > CONF_MAX_GROUPS ? CONF_MAX_GROUPS : nb)), dim3(64 * CONF_WAVES), 0, stream, label,
                     max_out, h, w, probs, lo, hi, ph, pw, (double)ph / (double)h, (double)pw / (double)w, thresh, band, table, out,
                     out_image, out_entropy, out_spread);
  return check_launch("label_confidence kernels");
}

}  // namespace unetdc
