// Deep (16-bit) images -> the 8-bit HWC image the flow takes: nearest-rank order statistics per channel
// by a two-level radix select, the integer window lo..hi -> 0..255, and the maximum over the planes of a stack.
//
//   ranks     value[ch][j] = the k_j-th smallest value of channel ch, k_j = max(1, ceil(p_j n / 10^6)), with below = #{v < value}
//             and equal = #{v == value}.  Five launches, nothing returns to the host in between:
//               fill_kernel<int>       the counters: zeros (wave_ops.h; the workspace may hold anything)
//               win_hist_kernel<.., 0> pass A: [c][256] histogram of the HIGH bytes
//               win_select_hi_kernel   per (ch, j): the bin that holds rank k_j, the count below the bin, the rank inside it
//               win_hist_kernel<.., 1> pass B: [nq][c][256] histograms of the LOW bytes of the values whose high byte is a
//                                      rank's bin; ranks of one channel that share a bin share one histogram (the first's)
//               win_select_lo_kernel   value / below / equal
//   histogram per workgroup in LDS, one copy per wave in pass A (4 x c x 256 words, 16 KB at most), one per workgroup in pass B
//             (nq x c x 256 words, 32 KB at most: four copies would not fit beside a second workgroup).  A lane holds eight values
//             of every channel (c consecutive 16-byte loads, so the channel of each element is known at compile time) and merges
//             runs of equal keys before it adds; where every lane of a wave holds one and the same key -- the usual case in a
//             smooth 12-bit micrograph, whose 512 neighbouring pixels share a high byte -- ONE lane adds the wave's count.  What
//             is left of same-address LDS atomics is the edges between intensity bands.  The nonzero bins go out as 32-bit
//             integer atomics (n < 2^30).  Integers only: the result depends on no order.
//   window    t = min(max(v, lo), hi) - lo, dst = (510 t + d) / (2 d) with d = hi - lo > 0 (round half up of 255 t / d; below
//             2^26), 0 for d <= 0; levels outside 0..65535 are clamped to it first.  Levels are read from device memory.
#include "kernels.h"
#include "wave_ops.h"

namespace unetdc {

constexpr int WIN_THREADS = 256;
constexpr int WIN_WAVES = WIN_THREADS / 64;
constexpr int WIN_HIST_MAX_GROUPS = 256;            // pass A / B: every workgroup flushes into the same few words (as sweep.hip)
constexpr int WIN_MAX_GROUPS = 1024;                // window, plane maximum
constexpr int WIN_MAX_RANKS = 8;
constexpr int WIN_MAX_PLANES = 256;
constexpr int WIN_PPM = 1000000;

struct WinRanks {                                   // by value in the kernel arguments
  int ppm[WIN_MAX_RANKS];
};

// per (ch, j), in the workspace: what the select of the high bytes leaves for pass B and the select of the low bytes
struct WinPlanes {
  int *hist_hi;       // [c][256]
  int *hist_lo;       // [nq][c][256]
  int *bin;           // [c][nq] the high byte of rank j
  int *below_bin;     // [c][nq] values of the channel in lower bins
  int *rem;           // [c][nq] the rank inside the bin, 1-based
  int *slot;          // [c][nq] the first j' of the channel with the same bin: its histogram serves rank j
};

static bool window_geometry_ok(int h, int w, int c) {
  return h >= 1 && w >= 1 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30) && c >= 1 && c <= 4;
}

static Layout<WinPlanes> ranks_layout(int h, int w, int c, int nq, void* workspace) {
  if (!(window_geometry_ok(h, w, c) && nq >= 1 && nq <= WIN_MAX_RANKS)) return {false, 0, {}};
  Carver cv(workspace);
  WinPlanes p;
  p.hist_hi = cv.take<int>((long)c * 256, 16);
  p.hist_lo = cv.take<int>((long)nq * c * 256, 16);
  p.bin = cv.take<int>((long)c * nq, 16);
  p.below_bin = cv.take<int>((long)c * nq, 16);
  p.rem = cv.take<int>((long)c * nq, 16);
  p.slot = cv.take<int>((long)c * nq, 16);
  return {true, cv.bytes(), p};
}
long u16_ranks_workspace_bytes(int h, int w, int c, int nq) { return ranks_layout(h, w, c, nq, nullptr).bytes; }

// The eight keys a lane holds for one channel (a negative key counts nowhere) -> hist.  All 64 lanes call it together.
__device__ __forceinline__ void win_add_keys(int* hist, const int (&key)[8], bool live, int lane) {
  bool uni = true;
#pragma unroll
  for (int i = 1; i < 8; ++i) uni = uni && key[i] == key[0];
  const unsigned long long alive = __ballot(live);
  if (!alive) return;
  const int first = __ffsll((long long)alive) - 1;
  const int lead = __shfl(key[0], first, 64);
  if (__all(!live || (uni && key[0] == lead))) {    // one key in the whole wave: one add
    if (lead >= 0 && lane == first) atomicAdd(&hist[lead], 8 * __popcll(alive));
    return;
  }
  if (!live) return;
  int run_key = key[0], run = 1;
#pragma unroll
  for (int i = 1; i < 8; ++i) {
    if (key[i] == run_key) { ++run; continue; }
    if (run_key >= 0) atomicAdd(&hist[run_key], run);
    run_key = key[i];
    run = 1;
  }
  if (run_key >= 0) atomicAdd(&hist[run_key], run);
}

// PASS 0: key = ch * 256 + (v >> 8), into hist_hi.  PASS 1: key = (slot * CN + ch) * 256 + (v & 255) for the values whose high
// byte is the bin of a rank of their channel, into hist_lo.  A lane takes CN consecutive 16-byte chunks = 8 pixels; the last
// npix % 8 pixels go one per thread of workgroup 0.
template <int CN, int PASS>
__global__ __launch_bounds__(WIN_THREADS) void win_hist_kernel(const unsigned short* __restrict__ src, long npix, int nq,
                                                               const int* __restrict__ sel_bin, const int* __restrict__ sel_slot,
                                                               int* __restrict__ out) {
  extern __shared__ int bins[];                     // PASS 0: [WIN_WAVES][CN * 256]; PASS 1: [nq][CN][256]
  __shared__ short lut[CN * 256];                   // PASS 1: high byte -> slot, -1 for a bin no rank lies in
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nbins = PASS == 0 ? CN * 256 : nq * CN * 256;
  const int copies = PASS == 0 ? WIN_WAVES : 1;
  for (int b = threadIdx.x; b < nbins * copies; b += WIN_THREADS) bins[b] = 0;
  if (PASS == 1) {
    for (int b = threadIdx.x; b < CN * 256; b += WIN_THREADS) lut[b] = -1;
    __syncthreads();
    if (threadIdx.x < CN * nq) {                    // [c][nq]; ranks that share a bin write the same slot
      const int ch = threadIdx.x / nq, b = sel_bin[threadIdx.x] & 255, s = sel_slot[threadIdx.x];
      if (s >= 0 && s < nq) lut[ch * 256 + b] = (short)s;
    }
  }
  __syncthreads();
  int* mine = bins + (PASS == 0 ? wave * nbins : 0);
  auto key_of = [&](int ch, unsigned v) -> int {
    if (PASS == 0) return ch * 256 + (int)(v >> 8);
    const int s = lut[ch * 256 + (int)(v >> 8)];
    return s < 0 ? -1 : (s * CN + ch) * 256 + (int)(v & 255u);
  };
  const long ngroups = npix / 8;
  for (long base = (long)blockIdx.x * WIN_THREADS; base < ngroups; base += (long)gridDim.x * WIN_THREADS) {
    const long g = base + threadIdx.x;              // the trip count is uniform in a workgroup: the ballots need all 64 lanes
    const bool live = g < ngroups;
    int key[CN][8];
    if (live) {
#pragma unroll
      for (int q = 0; q < CN; ++q) {
        const u32x4 a = ld16(src + (g * CN + q) * 8);
#pragma unroll
        for (int wI = 0; wI < 4; ++wI) {
          const unsigned word = a[wI];
#pragma unroll
          for (int hI = 0; hI < 2; ++hI) {
            const int e = 8 * q + 2 * wI + hI;      // element of the lane's 8 * CN: channel e % CN of pixel e / CN
            key[e % CN][e / CN] = key_of(e % CN, (word >> (16 * hI)) & 0xffffu);
          }
        }
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < CN; ++ch)
#pragma unroll
        for (int i = 0; i < 8; ++i) key[ch][i] = -1;
    }
#pragma unroll
    for (int ch = 0; ch < CN; ++ch) win_add_keys(mine, key[ch], live, lane);
  }
  if (blockIdx.x == 0) {
    const long p = ngroups * 8 + threadIdx.x;
    if (threadIdx.x < 8 && p < npix) {
#pragma unroll
      for (int ch = 0; ch < CN; ++ch) {
        const int k = key_of(ch, src[p * CN + ch]);
        if (k >= 0) atomicAdd(&mine[k], 1);
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += WIN_THREADS) {
    int s = 0;
    for (int q = 0; q < copies; ++q) s += bins[q * nbins + b];
    if (s) atomicAdd(&out[b], s);
  }
}

// One wave: the bin t of a 256-bin histogram with excl[t] < k <= excl[t] + hist[t] (excl: the counts of the lower bins).
// The lane that holds it returns true with (bin, below, count).  Four bins per lane, a wave scan of the lane sums.
__device__ __forceinline__ bool win_wave_select(const int* __restrict__ hist, int k, int lane, int& bin, int& below, int& count) {
  int v[4], s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { v[q] = hist[4 * lane + q]; s += v[q]; }
  int e = wave_incl_scan(s, lane) - s;
  bool found = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (!found && e < k && k <= e + v[q]) { found = true; bin = 4 * lane + q; below = e; count = v[q]; }
    e += v[q];
  }
  return found;
}

// one workgroup; task (ch, j) = ch * nq + j, a wave per task
__global__ __launch_bounds__(WIN_THREADS) void win_select_hi_kernel(const int* __restrict__ hist_hi, long npix, int c, int nq,
                                                                    const WinRanks r, int* __restrict__ sel_bin,
                                                                    int* __restrict__ sel_below, int* __restrict__ sel_rem,
                                                                    int* __restrict__ sel_slot) {
  __shared__ int s_bin[4 * WIN_MAX_RANKS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 4 * WIN_MAX_RANKS) s_bin[threadIdx.x] = -1 - threadIdx.x;      // no two alike, should a rank find no bin
  __syncthreads();
  for (int task = wave; task < c * nq; task += WIN_WAVES) {
    const int ch = task / nq, j = task - ch * nq;
    long long k = ((long long)r.ppm[j] * npix + (WIN_PPM - 1)) / WIN_PPM;
    k = k < 1 ? 1 : k;
    int bin = 0, below = 0, count = 0;
    if (win_wave_select(hist_hi + ch * 256, (int)k, lane, bin, below, count)) {
      s_bin[task] = bin;
      sel_bin[task] = bin;
      sel_below[task] = below;
      sel_rem[task] = (int)k - below;
    }
  }
  __syncthreads();
  if (threadIdx.x < c * nq) {
    const int task = threadIdx.x, ch = task / nq;
    int first = task;
    for (int t = task - 1; t >= ch * nq; --t) first = s_bin[t] == s_bin[task] ? t : first;
    sel_slot[task] = first - ch * nq;
  }
}

__global__ __launch_bounds__(WIN_THREADS) void win_select_lo_kernel(const int* __restrict__ hist_lo, int c, int nq,
                                                                    const int* __restrict__ sel_bin, const int* __restrict__ sel_below,
                                                                    const int* __restrict__ sel_rem, const int* __restrict__ sel_slot,
                                                                    int* __restrict__ out_value, int* __restrict__ out_below,
                                                                    int* __restrict__ out_equal) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int task = wave; task < c * nq; task += WIN_WAVES) {
    const int ch = task / nq;
    int slot = sel_slot[task];
    slot = slot < 0 ? 0 : (slot >= nq ? nq - 1 : slot);
    int lo = 0, below = 0, count = 0;
    if (win_wave_select(hist_lo + ((long)slot * c + ch) * 256, sel_rem[task], lane, lo, below, count)) {
      out_value[task] = (sel_bin[task] & 255) * 256 + lo;
      out_below[task] = sel_below[task] + below;
      out_equal[task] = count;
    }
  }
}

// dst = window(src): a lane takes CN 16-byte chunks (8 pixels) and writes 8 * CN * REP bytes in 8-byte stores.  REP = 3 only
// with CN = 1: the grey value three times.
template <int CN, int REP>
__global__ __launch_bounds__(WIN_THREADS) void win_apply_kernel(const unsigned short* __restrict__ src, long npix,
                                                                const int* __restrict__ levels, unsigned char* __restrict__ dst) {
  unsigned lo[CN], hi[CN], d[CN];
#pragma unroll
  for (int ch = 0; ch < CN; ++ch) {
    int a = levels[2 * ch], b = levels[2 * ch + 1];
    a = a < 0 ? 0 : (a > 65535 ? 65535 : a);
    b = b < 0 ? 0 : (b > 65535 ? 65535 : b);
    lo[ch] = (unsigned)a;
    hi[ch] = (unsigned)b;
    d[ch] = b > a ? (unsigned)(b - a) : 0u;
  }
  auto map = [&](int ch, unsigned v) -> unsigned {
    if (d[ch] == 0u) return 0u;
    const unsigned t = (v < lo[ch] ? lo[ch] : (v > hi[ch] ? hi[ch] : v)) - lo[ch];
    return (510u * t + d[ch]) / (2u * d[ch]);
  };
  const long ngroups = npix / 8;
  for (long g = (long)blockIdx.x * WIN_THREADS + threadIdx.x; g < ngroups; g += (long)gridDim.x * WIN_THREADS) {
    unsigned char o[8 * CN * REP];
#pragma unroll
    for (int q = 0; q < CN; ++q) {
      const u32x4 a = ld16(src + (g * CN + q) * 8);
#pragma unroll
      for (int wI = 0; wI < 4; ++wI) {
        const unsigned word = a[wI];
#pragma unroll
        for (int hI = 0; hI < 2; ++hI) {
          const int e = 8 * q + 2 * wI + hI;
          const unsigned char u = (unsigned char)map(e % CN, (word >> (16 * hI)) & 0xffffu);
#pragma unroll
          for (int rI = 0; rI < REP; ++rI) o[e * REP + rI] = u;
        }
      }
    }
    unsigned char* out = dst + g * (8 * CN * REP);
#pragma unroll
    for (int s = 0; s < CN * REP; ++s) {
      u32x2 pk;
      pk[0] = (unsigned)o[8 * s] | ((unsigned)o[8 * s + 1] << 8) | ((unsigned)o[8 * s + 2] << 16) | ((unsigned)o[8 * s + 3] << 24);
      pk[1] = (unsigned)o[8 * s + 4] | ((unsigned)o[8 * s + 5] << 8) | ((unsigned)o[8 * s + 6] << 16) | ((unsigned)o[8 * s + 7] << 24);
      *reinterpret_cast<u32x2*>(out + 8 * s) = pk;
    }
  }
  if (blockIdx.x == 0) {
    const long p = ngroups * 8 + threadIdx.x;
    if (threadIdx.x < 8 && p < npix) {
#pragma unroll
      for (int ch = 0; ch < CN; ++ch) {
        const unsigned char u = (unsigned char)map(ch, src[p * CN + ch]);
#pragma unroll
        for (int rI = 0; rI < REP; ++rI) dst[(p * CN + ch) * REP + rI] = u;
      }
    }
  }
}

// dst[i] = max over the planes of src[p][i].  VEC: npix % 8 == 0, so every plane starts on a 16-byte boundary.
template <bool VEC>
__global__ __launch_bounds__(WIN_THREADS) void win_planes_max_kernel(const unsigned short* __restrict__ src, int planes, long npix,
                                                                     unsigned short* __restrict__ dst) {
  const long items = VEC ? npix / 8 : npix;
  for (long i = (long)blockIdx.x * WIN_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * WIN_THREADS) {
    if (VEC) {
      u32x4 m = ld16(src + i * 8);
      for (int p = 1; p < planes; ++p) {
        const u32x4 a = ld16(src + (long)p * npix + i * 8);
#pragma unroll
        for (int wI = 0; wI < 4; ++wI) {
          const unsigned x = a[wI], y = m[wI];
          const unsigned l = (x & 0xffffu) > (y & 0xffffu) ? (x & 0xffffu) : (y & 0xffffu);
          const unsigned u = (x >> 16) > (y >> 16) ? (x >> 16) : (y >> 16);
          m[wI] = l | (u << 16);
        }
      }
      st16(dst + i * 8, m);
    } else {
      unsigned short m = src[i];
      for (int p = 1; p < planes; ++p) {
        const unsigned short a = src[(long)p * npix + i];
        m = a > m ? a : m;
      }
      dst[i] = m;
    }
  }
}

static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int launch_u16_ranks(const unsigned short* src, int h, int w, int c, const int* ppm, int nq, void* workspace, long workspace_bytes,
                     int* out_value, int* out_below, int* out_equal, hipStream_t stream) {
  UNETDC_REQUIRE(src && ppm && workspace && out_value && out_below && out_equal, "u16_ranks: null pointer");
  const auto lay = ranks_layout(h, w, c, nq, workspace);
  UNETDC_REQUIRE(lay.ok, "u16_ranks: bad geometry %dx%dx%d, %d ranks (sides 1..16384, h * w < 2^30, 1..4 channels, 1..%d ranks)", h, w,
                 c, nq, WIN_MAX_RANKS);
  WinRanks r = {};
  for (int j = 0; j < nq; ++j) {
    UNETDC_REQUIRE(ppm[j] >= 0 && ppm[j] <= WIN_PPM, "u16_ranks: rank %d = %d outside 0..%d parts per million", j, ppm[j], WIN_PPM);
    r.ppm[j] = ppm[j];
  }
  if (int rc = require_workspace("u16_ranks", workspace_bytes, lay.bytes)) return rc;
  UNETDC_REQUIRE(aligned16(src) && aligned16(workspace), "u16_ranks: the image and the workspace must be 16-byte aligned");
  UNETDC_REQUIRE(((uintptr_t)out_value | (uintptr_t)out_below | (uintptr_t)out_equal) % 4 == 0, "u16_ranks: the outputs must be 4-byte aligned");
  const WinPlanes p = lay.planes;
  const long npix = (long)h * w;
  const int counters = c * 256 * (1 + nq);          // hist_hi and hist_lo are neighbours in the layout
  launch_fill(p.hist_hi, (long)counters, 0, grid_for(counters, WIN_THREADS, 64), stream);
  const dim3 grid(grid_for(npix / 8, WIN_THREADS, WIN_HIST_MAX_GROUPS)), block(WIN_THREADS);
  const int lds_hi = WIN_WAVES * c * 256 * 4, lds_lo = nq * c * 256 * 4;
  auto hist = [&](auto cn, auto pass) {
    constexpr int CN = decltype(cn)::value, PASS = decltype(pass)::value;
    hipLaunchKernelGGL((win_hist_kernel<CN, PASS>), grid, block, PASS == 0 ? lds_hi : lds_lo, stream, src, npix, nq, p.bin, p.slot,
                       PASS == 0 ? p.hist_hi : p.hist_lo);
  };
  auto per_channels = [&](auto pass) {
    if (c == 1) hist(std::integral_constant<int, 1>{}, pass);
    else if (c == 2) hist(std::integral_constant<int, 2>{}, pass);
    else if (c == 3) hist(std::integral_constant<int, 3>{}, pass);
    else hist(std::integral_constant<int, 4>{}, pass);
  };
  per_channels(std::integral_constant<int, 0>{});
  hipLaunchKernelGGL(win_select_hi_kernel, dim3(1), block, 0, stream, p.hist_hi, npix, c, nq, r, p.bin, p.below_bin, p.rem, p.slot);
  per_channels(std::integral_constant<int, 1>{});
  hipLaunchKernelGGL(win_select_lo_kernel, dim3(1), block, 0, stream, p.hist_lo, c, nq, p.bin, p.below_bin, p.rem, p.slot, out_value,
                     out_below, out_equal);
  return check_launch("u16_ranks kernels");
}

int launch_window_u16_to_u8(const unsigned short* src, int h, int w, int c, const int* levels, unsigned char* dst, int dc,
                            hipStream_t stream) {
  UNETDC_REQUIRE(src && levels && dst, "window_u16_to_u8: null pointer");
  UNETDC_REQUIRE(window_geometry_ok(h, w, c), "window_u16_to_u8: bad geometry %dx%dx%d (sides 1..16384, h * w < 2^30, 1..4 channels)", h,
                 w, c);
  UNETDC_REQUIRE(dc == c || (dc == 3 && c == 1), "window_u16_to_u8: %d output channels from %d (the same number, or 3 from 1)", dc, c);
  UNETDC_REQUIRE(aligned16(src) && aligned16(dst), "window_u16_to_u8: the images must be 16-byte aligned");
  UNETDC_REQUIRE(reinterpret_cast<uintptr_t>(levels) % 4 == 0, "window_u16_to_u8: the levels must be 4-byte aligned");
  const long npix = (long)h * w;
  const dim3 grid(grid_for(npix / 8, WIN_THREADS, WIN_MAX_GROUPS)), block(WIN_THREADS);
  if (c == 1 && dc == 3) hipLaunchKernelGGL((win_apply_kernel<1, 3>), grid, block, 0, stream, src, npix, levels, dst);
  else if (c == 1) hipLaunchKernelGGL((win_apply_kernel<1, 1>), grid, block, 0, stream, src, npix, levels, dst);
  else if (c == 2) hipLaunchKernelGGL((win_apply_kernel<2, 1>), grid, block, 0, stream, src, npix, levels, dst);
  else if (c == 3) hipLaunchKernelGGL((win_apply_kernel<3, 1>), grid, block, 0, stream, src, npix, levels, dst);
  else hipLaunchKernelGGL((win_apply_kernel<4, 1>), grid, block, 0, stream, src, npix, levels, dst);
  return check_launch("win_apply_kernel");
}

int launch_planes_max_u16(const unsigned short* src, int planes, int h, int w, unsigned short* dst, hipStream_t stream) {
  UNETDC_REQUIRE(src && dst, "planes_max_u16: null pointer");
  UNETDC_REQUIRE(window_geometry_ok(h, w, 1) && planes >= 1 && planes <= WIN_MAX_PLANES,
                 "planes_max_u16: bad geometry %d planes of %dx%d (1..%d planes, sides 1..16384, h * w < 2^30)", planes, h, w,
                 WIN_MAX_PLANES);
  UNETDC_REQUIRE(aligned16(src) && aligned16(dst), "planes_max_u16: the images must be 16-byte aligned");
  const long npix = (long)h * w;
  const dim3 block(WIN_THREADS);
  if (npix % 8 == 0)
    hipLaunchKernelGGL(win_planes_max_kernel<true>, dim3(grid_for(npix / 8, WIN_THREADS, WIN_MAX_GROUPS)), block, 0, stream, src, planes,
                       npix, dst);
  else
    hipLaunchKernelGGL(win_planes_max_kernel<false>, dim3(grid_for(npix, WIN_THREADS, WIN_MAX_GROUPS)), block, 0, stream, src, planes,
                       npix, dst);
  return check_launch("win_planes_max_kernel");
}

}  // namespace unetdc
