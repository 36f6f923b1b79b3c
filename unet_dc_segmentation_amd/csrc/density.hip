// Radial and spatial droplet density maps on the GPU, the analysis of the reference's quantify_pipline.py:
//   roi = generate_roi_mask(orig)                         gray -> GaussianBlur 15x15 -> Otsu -> MORPH_CLOSE/OPEN 15x15   :44-51
//   cx, cy = centroid of cv2.moments(roi), (ow//2, oh//2) when m00 == 0                                                  :133-135
//   radial  = get_targets(mask, roi, nb_layers, cy, cx)   droplets per concentric ring, painted on the ring's ROI pixels :61-91
//   spatial = gaussian_filter(mask, s) / (gaussian_filter(roi, s) + 1e-5) * 100                                          :93-97
//   plt.imsave(normalize(map), cmap="hot")                -> uint8 colormap index planes                                 :141-142
// restated exactly (the yardstick is utils/density.py; cv2 is not available to this build, so parity against cv2 is unpinned,
// as for the rolling ball):
//   density_blur_kernel   gray = (4899 R + 9617 G + 1868 B + 8192) >> 14, then OpenCV's bit-exact 8-bit GaussianBlur with the
//                         15 fixed-point taps DENS_BLUR_TAPS, BORDER_REFLECT_101: out = (sum_ij k_i k_j g + 32768) >> 16 (exact
//                         integers); the 256-bin histogram of the result (LDS, then one global atomic per bin and block)
//   density_otsu_kernel   OpenCV's double-precision Otsu scan over that histogram, threshold to a device word
//   morph_kernel (x4)     close then open with the 15 x 15 rectangle, run on the BLURRED plane (launch_morph_rect): erosion and
//                         dilation commute with the monotone step `v > t`, so open(close(blur > t)) == (open(close(blur)) > t)
//                         -- outside pixels do not take part in either form, and t <= 254 (Otsu never picks 255) -- and the
//                         morphology does not wait for the threshold
//   density_rows_kernel   roi = opened > t; per row: ROI pixel count, sum of x, first / last ROI column (no atomics)
//   density_rings_kernel  one workgroup: moments, centroid, maximum squared ROI distance (it is reached at a row's first or last
//                         ROI pixel), np.linspace ring bounds, per-droplet distance and ring -> ring counts
//   density_radial_kernel ring index and radial value per pixel, min / max of the map
//   density_gauss0/1      scipy.ndimage.gaussian_filter: axis 0 then axis 1, fp64 accumulation in scipy's order (centre tap,
//                         then symmetric pairs from the outermost inwards), float32 between the axes, mode "reflect"; then
//                         the float32 ratio * 100 and min / max of the map
//   density_index_kernel  normalize + plt.imsave's colormap rule: index = min(int(t * 256), 255), 0 for a constant map
// Floating point: hipcc contracts a * b + c into one FMA (-ffp-contract=fast) even across __fmul_rn / __fadd_rn; every product
// that feeds an addition goes through dens_opaque (an empty asm), which keeps the two roundings numpy and OpenCV perform.
// Everything here is byte / integer / scalar-fp64 work on ~1.4 Mpixel planes: bound by HBM traffic and launch count.
#include "kernels.h"

#include <math.h>

#include "../../include/unetdc_hip.h"

namespace unetdc {

constexpr int DENSITY_MIN_SIDE = UNETDC_DENSITY_MIN_SIDE;
constexpr int DENSITY_MAX_LAYERS = UNETDC_DENSITY_MAX_LAYERS;
constexpr int DENSITY_MAX_RADIUS = UNETDC_DENSITY_MAX_RADIUS;
constexpr int DENS_THREADS = 256;
constexpr int DENS_BLUR_K = 15, DENS_BLUR_R = 7;
constexpr int DENS_TH = 32, DENS_TW = 64;                    // blur output tile
constexpr int DENS_PH = DENS_TH + 2 * DENS_BLUR_R, DENS_PW = DENS_TW + 2 * DENS_BLUR_R;
constexpr int DENS_MORPH_K = 15;
constexpr int DENS_RINGS_THREADS = 1024;

__constant__ int DENS_BLUR_TAPS[DENS_BLUR_K] = {1, 3, 6, 12, 20, 30, 36, 40, 36, 30, 20, 12, 6, 3, 1};

struct DensTaps {
  double w[DENSITY_MAX_RADIUS + 1];
};

__device__ __forceinline__ double dens_opaque(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), n >= 2, any distance from the image
__device__ __forceinline__ int dens_reflect101(int i, int n) {
  const int p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// scipy.ndimage mode "reflect" (dcba|abcd|dcba), n >= 1, any distance from the image
__device__ __forceinline__ int dens_reflect(int i, int n) {
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

__device__ __forceinline__ double dens_sqrt(double v) { return sqrt(v); }    // correctly rounded (tests/test_gpu_density.py)

// the per-image scalars between the kernels (workspace)
struct DensScratch {
  int hist[256];
  int thresh;
  int pad_;
  unsigned long long maxd2;
};

__global__ void density_init_kernel(DensScratch* sc, unetdc_density_stats* st) {
  const int t = threadIdx.x;
  sc->hist[t] = 0;
  if (t == 0) {
    st->radial_min_bits = 0xFFFFFFFFu;
    st->radial_max_bits = 0u;
    st->spatial_min_bits = 0xFFFFFFFFu;
    st->spatial_max_bits = 0u;
  }
}

// grid (ceil(W / 64), ceil(H / 32)), 256 threads: gray of the (32 + 14) x (64 + 14) patch (reflect-101 indices), horizontal
// pass into LDS, vertical pass, rounding shift; 8 outputs per thread
__global__ __launch_bounds__(DENS_THREADS) void density_blur_kernel(const unsigned char* __restrict__ rgb, int H, int W,
                                                                    unsigned char* __restrict__ blur, int* __restrict__ hist) {
  __shared__ int g[DENS_PH][DENS_PW];
  __shared__ int hrow[DENS_PH][DENS_TW];
  __shared__ int lh[256];
  const int tid = threadIdx.x;
  const int y0 = blockIdx.y * DENS_TH, x0 = blockIdx.x * DENS_TW;
  lh[tid] = 0;
  for (int i = tid; i < DENS_PH * DENS_PW; i += DENS_THREADS) {
    const int py = i / DENS_PW, px = i - py * DENS_PW;
    const int gy = dens_reflect101(y0 + py - DENS_BLUR_R, H), gx = dens_reflect101(x0 + px - DENS_BLUR_R, W);
    const unsigned char* p = rgb + ((long)gy * W + gx) * 3;
    g[py][px] = (4899 * p[0] + 9617 * p[1] + 1868 * p[2] + 8192) >> 14;
  }
  __syncthreads();
  for (int i = tid; i < DENS_PH * DENS_TW; i += DENS_THREADS) {
    const int py = i / DENS_TW, px = i - py * DENS_TW;
    int s = 0;
#pragma unroll
    for (int k = 0; k < DENS_BLUR_K; ++k) s += DENS_BLUR_TAPS[k] * g[py][px + k];
    hrow[py][px] = s;
  }
  __syncthreads();
  for (int i = tid; i < DENS_TH * DENS_TW; i += DENS_THREADS) {
    const int ty = i / DENS_TW, tx = i - ty * DENS_TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    int s = 0;
#pragma unroll
    for (int k = 0; k < DENS_BLUR_K; ++k) s += DENS_BLUR_TAPS[k] * hrow[ty + k][tx];
    const int v = (s + 32768) >> 16;                        // <= (255 * 65536 + 32768) >> 16 = 255
    blur[(long)y * W + x] = (unsigned char)v;
    atomicAdd(&lh[v], 1);
  }
  __syncthreads();
  if (lh[tid]) atomicAdd(&hist[tid], lh[tid]);
}

// cv::threshold(..., THRESH_OTSU) on 8-bit data (getThreshVal_Otsu_8u): the wave stages the histogram in LDS, then one thread
// runs the 256 dependent steps in double.  Every product that feeds an addition is opaque: p_i = h_i * scale fused into
// q1 += p_i (one rounding instead of two) moves the threshold wherever two splits tie exactly (tests: the stripe image).
__global__ __launch_bounds__(64) void density_otsu_kernel(const DensScratch* __restrict__ scin, DensScratch* sc, long npix,
                                                          unetdc_density_stats* st) {
  __shared__ double h[256];
  for (int i = threadIdx.x; i < 256; i += 64) h[i] = (double)scin->hist[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double scale = 1.0 / (double)npix;
  double mu = 0.0;
  for (int i = 0; i < 256; ++i) mu += dens_opaque((double)i * h[i]);
  mu *= scale;
  double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
  int max_val = 0;
  const double feps = 1.1920928955078125e-07;                // FLT_EPSILON
  for (int i = 0; i < 256; ++i) {
    const double p_i = dens_opaque(h[i] * scale);
    mu1 *= q1;
    q1 += p_i;
    const double q2 = 1.0 - q1;
    if (fmin(q1, q2) < feps || fmax(q1, q2) > 1.0 - feps) continue;
    mu1 = (mu1 + dens_opaque((double)i * p_i)) / q1;
    const double mu2 = (mu - dens_opaque(q1 * mu1)) / q2;
    const double d = mu1 - mu2;
    const double sigma = q1 * q2 * d * d;
    if (sigma > max_sigma) {
      max_sigma = sigma;
      max_val = i;
    }
  }
  sc->thresh = max_val;
  st->otsu_threshold = max_val;
}

// one block per row: roi = opened > t (written as 0 / 1), and the row's ROI count, sum of x, first and last ROI column
__global__ __launch_bounds__(DENS_THREADS) void density_rows_kernel(const unsigned char* __restrict__ opened, int W,
                                                                    const DensScratch* __restrict__ sc,
                                                                    unsigned char* __restrict__ roi, int* __restrict__ row_cnt,
                                                                    long long* __restrict__ row_sumx,
                                                                    int* __restrict__ row_xmin, int* __restrict__ row_xmax) {
  __shared__ int s_cnt[DENS_THREADS / 64], s_min[DENS_THREADS / 64], s_max[DENS_THREADS / 64];
  __shared__ long long s_sum[DENS_THREADS / 64];
  const int y = blockIdx.x, t = sc->thresh;
  int cnt = 0, xmin = W, xmax = -1;
  long long sum = 0;
  for (int x = threadIdx.x; x < W; x += DENS_THREADS) {
    const int on = opened[(long)y * W + x] > t;
    roi[(long)y * W + x] = (unsigned char)on;
    if (on) {
      ++cnt;
      sum += x;
      xmin = x < xmin ? x : xmin;
      xmax = x;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sum += __shfl_xor(sum, o, 64);
    const int a = __shfl_xor(xmin, o, 64), b = __shfl_xor(xmax, o, 64);
    xmin = a < xmin ? a : xmin;
    xmax = b > xmax ? b : xmax;
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_cnt[wv] = cnt; s_sum[wv] = sum; s_min[wv] = xmin; s_max[wv] = xmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0, mn = W, mx = -1;
    long long sm = 0;
    for (int k = 0; k < DENS_THREADS / 64; ++k) {
      c += s_cnt[k];
      sm += s_sum[k];
      mn = s_min[k] < mn ? s_min[k] : mn;
      mx = s_max[k] > mx ? s_max[k] : mx;
    }
    row_cnt[y] = c;
    row_sumx[y] = sm;
    row_xmin[y] = mn;
    row_xmax[y] = mx;
  }
}

template <typename T>
__device__ __forceinline__ T dens_block_sum(T v, T* red) {          // DENS_RINGS_THREADS threads, result in every thread
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = 0;
  for (int k = 0; k < DENS_RINGS_THREADS / 64; ++k) s += red[k];
  return s;
}

// number of bounds b[0..L) below d, minus one: the ring whose half-open interval (b[i], b[i + 1]] holds d, or -1
__device__ __forceinline__ int dens_ring_of(const double* b, int L, double d) {
  int lo = 0, hi = L;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b[mid] < d) lo = mid + 1;
    else hi = mid;
  }
  const int i = lo - 1;
  return (i >= 0 && d <= b[i + 1]) ? i : -1;
}

// one workgroup of 1024 threads
__global__ __launch_bounds__(DENS_RINGS_THREADS) void density_rings_kernel(
    int H, int W, const int* __restrict__ row_cnt, const long long* __restrict__ row_sumx, const int* __restrict__ row_xmin,
    const int* __restrict__ row_xmax, const int* __restrict__ dcount, const int* __restrict__ darea,
    const long long* __restrict__ dsumy, const long long* __restrict__ dsumx, int dcap, int L, double* __restrict__ bounds,
    DensScratch* sc, unetdc_density_stats* st) {
  __shared__ long long red[DENS_RINGS_THREADS / 64];
  __shared__ unsigned long long redu[DENS_RINGS_THREADS / 64];
  __shared__ double b[DENSITY_MAX_LAYERS + 1];
  __shared__ int cnt[DENSITY_MAX_LAYERS];
  const int tid = threadIdx.x;
  long long m00 = 0, m10 = 0, m01 = 0;
  for (int y = tid; y < H; y += DENS_RINGS_THREADS) {
    m00 += row_cnt[y];
    m10 += row_sumx[y];
    m01 += (long long)y * row_cnt[y];
  }
  m00 = dens_block_sum(m00, red);
  m10 = dens_block_sum(m10, red);
  m01 = dens_block_sum(m01, red);
  // cx = int(M["m10"] / M["m00"]): double division, truncation
  const int cx = m00 ? (int)((double)m10 / (double)m00) : W / 2;
  const int cy = m00 ? (int)((double)m01 / (double)m00) : H / 2;
  unsigned long long d2 = 0;
  for (int y = tid; y < H; y += DENS_RINGS_THREADS) {
    if (!row_cnt[y]) continue;
    const long long dy = y - cy, a = row_xmin[y] - cx, c = row_xmax[y] - cx;
    const long long dx2 = a * a > c * c ? a * a : c * c;
    const unsigned long long v = (unsigned long long)(dx2 + dy * dy);
    d2 = v > d2 ? v : d2;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = __shfl_xor(d2, o, 64);
    d2 = v > d2 ? v : d2;
  }
  __syncthreads();
  if ((tid & 63) == 0) redu[tid >> 6] = d2;
  __syncthreads();
  for (int k = 0; k < DENS_RINGS_THREADS / 64; ++k) d2 = redu[k] > d2 ? redu[k] : d2;
  // np.linspace(0, maxd, L + 1): step = maxd / L, b_i = i * step, b_L = maxd
  const double maxd = dens_sqrt((double)d2);
  const double step = maxd / (double)L;
  for (int i = tid; i <= L; i += DENS_RINGS_THREADS) b[i] = i < L ? (double)i * step : maxd;
  for (int i = tid; i < L; i += DENS_RINGS_THREADS) cnt[i] = 0;
  __syncthreads();
  int n = *dcount;
  n = n < dcap ? n : dcap;
  if (m00) {
    for (int k = tid; k < n; k += DENS_RINGS_THREADS) {
      const double a = (double)darea[k];
      const double dx = (double)dsumx[k] / a - (double)cx, dy = (double)dsumy[k] / a - (double)cy;
      const double d = dens_sqrt(dens_opaque(dx * dx) + dens_opaque(dy * dy));
      const int r = dens_ring_of(b, L, d);
      if (r >= 0) atomicAdd(&cnt[r], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i <= L; i += DENS_RINGS_THREADS) bounds[i] = b[i];
  for (int i = tid; i < DENSITY_MAX_LAYERS; i += DENS_RINGS_THREADS) st->ring_count[i] = i < L ? cnt[i] : 0;
  if (tid == 0) {
    st->roi_area = m00;
    st->m10 = m10;
    st->m01 = m01;
    st->cx = cx;
    st->cy = cy;
    st->nb_layers = L;
    st->ndroplets = *dcount;
    st->max_ring_distance = maxd;
    sc->maxd2 = d2;
  }
}

__device__ __forceinline__ void dens_minmax_commit(unsigned mn, unsigned mx, unsigned* gmn, unsigned* gmx) {
  __shared__ unsigned smn[DENS_THREADS / 64], smx[DENS_THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < DENS_THREADS / 64; ++k) {
      mn = smn[k] < mn ? smn[k] : mn;
      mx = smx[k] > mx ? smx[k] : mx;
    }
    atomicMin(gmn, mn);
    atomicMax(gmx, mx);
  }
}

// ring index (0 = no ring, i + 1 = ring i) and the radial map value (the ring's droplet count) of every pixel
__global__ __launch_bounds__(DENS_THREADS) void density_radial_kernel(const unsigned char* __restrict__ roi, int H, int W,
                                                                      const double* __restrict__ bounds, int L,
                                                                      unetdc_density_stats* st,
                                                                      unsigned char* __restrict__ ring,
                                                                      float* __restrict__ radial) {
  __shared__ double b[DENSITY_MAX_LAYERS + 1];
  __shared__ float val[DENSITY_MAX_LAYERS];
  for (int i = threadIdx.x; i <= L; i += DENS_THREADS) b[i] = bounds[i];
  for (int i = threadIdx.x; i < L; i += DENS_THREADS) val[i] = (float)st->ring_count[i];
  __syncthreads();
  const int cx = st->cx, cy = st->cy;
  const long n = (long)H * W;
  unsigned mn = 0xFFFFFFFFu, mx = 0u;
  for (long p = (long)blockIdx.x * DENS_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * DENS_THREADS) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    int r = -1;
    if (roi[p]) {
      const long long dx = x - cx, dy = y - cy;
      r = dens_ring_of(b, L, dens_sqrt((double)(dx * dx + dy * dy)));     // integer d^2: exact in double
    }
    const float v = r >= 0 ? val[r] : 0.0f;
    ring[p] = (unsigned char)(r + 1);
    radial[p] = v;
    const unsigned u = __float_as_uint(v);
    mn = u < mn ? u : mn;
    mx = u > mx ? u : mx;
  }
  dens_minmax_commit(mn, mx, &st->radial_min_bits, &st->radial_max_bits);
}

// gaussian_filter along axis 0 of the mask and the ROI: out(y, x) = float32(v(y) w0 + sum_{j = r..1} (v(y - j) + v(y + j)) w_j)
__global__ __launch_bounds__(DENS_THREADS) void density_gauss0_kernel(const unsigned char* __restrict__ mask,
                                                                      const unsigned char* __restrict__ roi, int H, int W,
                                                                      const DensTaps tp, int R, float* __restrict__ gm,
                                                                      float* __restrict__ gr) {
  const long n = (long)H * W;
  for (long p = (long)blockIdx.x * DENS_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * DENS_THREADS) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    double am = dens_opaque((double)mask[p] * tp.w[0]), ar = dens_opaque((double)roi[p] * tp.w[0]);
    const bool inner = y >= R && y + R < H;                  // no reflection needed (uniform over most of the grid)
    for (int j = R; j >= 1; --j) {
      const long i0 = inner ? p - (long)j * W : (long)dens_reflect(y - j, H) * W + x;
      const long i1 = inner ? p + (long)j * W : (long)dens_reflect(y + j, H) * W + x;
      am += dens_opaque((double)(mask[i0] + mask[i1]) * tp.w[j]);
      ar += dens_opaque((double)(roi[i0] + roi[i1]) * tp.w[j]);
    }
    gm[p] = (float)am;
    gr[p] = (float)ar;
  }
}

// axis 1 of both planes, then spatial = gm / (gr + 1e-5) * 100 in float32, and min / max of the map
__global__ __launch_bounds__(DENS_THREADS) void density_gauss1_kernel(const float* __restrict__ gm, const float* __restrict__ gr,
                                                                      int H, int W, const DensTaps tp, int R,
                                                                      unetdc_density_stats* st, float* __restrict__ spatial) {
  const long n = (long)H * W;
  unsigned mn = 0xFFFFFFFFu, mx = 0u;
  for (long p = (long)blockIdx.x * DENS_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * DENS_THREADS) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const long row = (long)y * W;
    double am = dens_opaque((double)gm[p] * tp.w[0]), ar = dens_opaque((double)gr[p] * tp.w[0]);
    const bool inner = x >= R && x + R < W;
    for (int j = R; j >= 1; --j) {
      const long i0 = inner ? p - j : row + dens_reflect(x - j, W), i1 = inner ? p + j : row + dens_reflect(x + j, W);
      am += dens_opaque(((double)gm[i0] + (double)gm[i1]) * tp.w[j]);
      ar += dens_opaque(((double)gr[i0] + (double)gr[i1]) * tp.w[j]);
    }
    const float fm = (float)am, fr = (float)ar;
    const float v = fm / (fr + 1e-5f) * 100.0f;              // three float32 roundings: add, divide, multiply
    spatial[p] = v;
    const unsigned u = __float_as_uint(v);                   // v >= 0: the bit patterns order like the values
    mn = u < mn ? u : mn;
    mx = u > mx ? u : mx;
  }
  dens_minmax_commit(mn, mx, &st->spatial_min_bits, &st->spatial_max_bits);
}

__device__ __forceinline__ unsigned char dens_index(float v, float mn, float mx) {
  if (!(mx > mn)) return 0;                                  // normalize leaves a constant map; imsave maps it to lut[0]
  const float t = (v - mn) / (mx - mn);
  const int i = (int)(t * 256.0f);
  return (unsigned char)(i < 255 ? i : 255);
}

__global__ __launch_bounds__(DENS_THREADS) void density_index_kernel(const float* __restrict__ radial,
                                                                     const float* __restrict__ spatial, long n,
                                                                     const unetdc_density_stats* __restrict__ st,
                                                                     unsigned char* __restrict__ ri,
                                                                     unsigned char* __restrict__ si) {
  const float rmn = __uint_as_float(st->radial_min_bits), rmx = __uint_as_float(st->radial_max_bits);
  const float smn = __uint_as_float(st->spatial_min_bits), smx = __uint_as_float(st->spatial_max_bits);
  for (long p = (long)blockIdx.x * DENS_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * DENS_THREADS) {
    ri[p] = dens_index(radial[p], rmn, rmx);
    si[p] = dens_index(spatial[p], smn, smx);
  }
}

__global__ void density_sqrt_kernel(const long long* __restrict__ x, double* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = dens_sqrt((double)x[i]);
}

// workspace layout: every part rounded to 256 bytes
struct DensPlanes {
  DensScratch* sc;
  int* rcnt;
  long long* rsum;
  int *rmin, *rmax;
  double* bounds;
  unsigned char *blur, *m1, *m2, *roi, *ring;
  float *radial, *g0m, *g0r, *spatial;
};
static Layout<DensPlanes> dens_layout(int h, int w, void* workspace) {
  if (!(h >= DENSITY_MIN_SIDE && w >= DENSITY_MIN_SIDE && (long)h * w < (1L << 30))) return {false, 0, {}};
  const long n = (long)h * w;
  Carver c(workspace);
  DensPlanes p;
  p.sc = c.take<DensScratch>(1, 256);
  p.rcnt = c.take<int>(h, 256);
  p.rsum = c.take<long long>(h, 256);
  p.rmin = c.take<int>(h, 256);
  p.rmax = c.take<int>(h, 256);
  p.bounds = c.take<double>(DENSITY_MAX_LAYERS + 1, 256);
  p.blur = c.take<unsigned char>(n, 256);
  p.m1 = c.take<unsigned char>(n, 256);
  p.m2 = c.take<unsigned char>(n, 256);
  p.roi = c.take<unsigned char>(n, 256);
  p.ring = c.take<unsigned char>(n, 256);
  p.radial = c.take<float>(n, 256);
  p.g0m = c.take<float>(n, 256);
  p.g0r = c.take<float>(n, 256);
  p.spatial = c.take<float>(n, 256);
  return {true, c.bytes(), p};
}
long density_workspace_bytes(int h, int w) { return dens_layout(h, w, nullptr).bytes; }

int launch_density_maps(const unsigned char* rgb, const unsigned char* mask, int h, int w, const int* dcount, const int* darea,
                        const long long* dsumy, const long long* dsumx, int dcap, int nb_layers, double sigma,
                        const double* taps, void* workspace, long workspace_bytes, unetdc_density_stats* stats,
                        unsigned char* radial_index, unsigned char* spatial_index, unsigned char* out_blur,
                        unsigned char* out_roi, unsigned char* out_ring, float* out_radial, float* out_spatial,
                        hipStream_t stream) {
  UNETDC_REQUIRE(rgb && mask && dcount && darea && dsumy && dsumx && taps && workspace && stats && radial_index &&
                     spatial_index,
                 "density_maps: null pointer");
  const auto lay = dens_layout(h, w, workspace);
  UNETDC_REQUIRE(lay.ok, "density_maps: bad geometry h=%d w=%d (each side >= %d, h * w < 2^30)", h, w, DENSITY_MIN_SIDE);
  UNETDC_REQUIRE(nb_layers >= 1 && nb_layers <= DENSITY_MAX_LAYERS, "density_maps: nb_layers=%d outside 1..%d", nb_layers,
                 DENSITY_MAX_LAYERS);
  UNETDC_REQUIRE(dcap >= 0, "density_maps: bad droplet capacity %d", dcap);
  UNETDC_REQUIRE(isfinite(sigma) && sigma > 0.0 && (int)(4.0 * sigma + 0.5) <= DENSITY_MAX_RADIUS,
                 "density_maps: bad sigma %g (needs 0 < sigma and int(4 sigma + 0.5) <= %d)", sigma, DENSITY_MAX_RADIUS);
  const int R = (int)(4.0 * sigma + 0.5);
  DensTaps tp;
  for (int j = 0; j <= DENSITY_MAX_RADIUS; ++j) tp.w[j] = j <= R ? taps[j] : 0.0;
  for (int j = 0; j <= R; ++j) UNETDC_REQUIRE(isfinite(tp.w[j]) && tp.w[j] >= 0.0, "density_maps: bad tap %d", j);
  if (int rc = require_workspace("density_maps", workspace_bytes, lay.bytes)) return rc;
  DensPlanes p = lay.planes;                                // a plane the caller wants takes the place of the workspace's
  if (out_blur) p.blur = out_blur;
  if (out_roi) p.roi = out_roi;
  if (out_ring) p.ring = out_ring;
  if (out_radial) p.radial = out_radial;
  if (out_spatial) p.spatial = out_spatial;
  const auto [sc, rcnt, rsum, rmin, rmax, bounds, blur, m1, m2, roi, ring, radial, g0m, g0r, spatial] = p;
  const long n = (long)h * w;
  const dim3 flat(grid_for(n, DENS_THREADS, 4096));

  hipLaunchKernelGGL(density_init_kernel, dim3(1), dim3(256), 0, stream, sc, stats);
  hipLaunchKernelGGL(density_blur_kernel, dim3((w + DENS_TW - 1) / DENS_TW, (h + DENS_TH - 1) / DENS_TH), dim3(DENS_THREADS), 0,
                     stream, rgb, h, w, blur, sc->hist);
  hipLaunchKernelGGL(density_otsu_kernel, dim3(1), dim3(64), 0, stream, sc, sc, n, stats);
  // MORPH_CLOSE = erode(dilate(.)), MORPH_OPEN = dilate(erode(.)), all with the 15 x 15 rectangle
  int rc = launch_morph_rect(blur, m1, h, w, DENS_MORPH_K, true, stream);
  if (rc == UNETDC_OK) rc = launch_morph_rect(m1, m2, h, w, DENS_MORPH_K, false, stream);
  if (rc == UNETDC_OK) rc = launch_morph_rect(m2, m1, h, w, DENS_MORPH_K, false, stream);
  if (rc == UNETDC_OK) rc = launch_morph_rect(m1, m2, h, w, DENS_MORPH_K, true, stream);
  if (rc != UNETDC_OK) return rc;
  hipLaunchKernelGGL(density_rows_kernel, dim3(h), dim3(DENS_THREADS), 0, stream, m2, w, sc, roi, rcnt, rsum, rmin, rmax);
  hipLaunchKernelGGL(density_rings_kernel, dim3(1), dim3(DENS_RINGS_THREADS), 0, stream, h, w, rcnt, rsum, rmin, rmax, dcount,
                     darea, dsumy, dsumx, dcap, nb_layers, bounds, sc, stats);
  hipLaunchKernelGGL(density_radial_kernel, flat, dim3(DENS_THREADS), 0, stream, roi, h, w, bounds, nb_layers, stats, ring, radial);
  hipLaunchKernelGGL(density_gauss0_kernel, flat, dim3(DENS_THREADS), 0, stream, mask, roi, h, w, tp, R, g0m, g0r);
  hipLaunchKernelGGL(density_gauss1_kernel, flat, dim3(DENS_THREADS), 0, stream, g0m, g0r, h, w, tp, R, stats, spatial);
  hipLaunchKernelGGL(density_index_kernel, flat, dim3(DENS_THREADS), 0, stream, radial, spatial, n, stats, radial_index,
                     spatial_index);
  return check_launch("density kernels");
}

int launch_density_sqrt(const long long* x, double* out, long n, hipStream_t stream) {
  UNETDC_REQUIRE(x && out && n >= 0, "density_sqrt: bad arguments");
  if (n == 0) return UNETDC_OK;
  hipLaunchKernelGGL(density_sqrt_kernel, dim3(grid_for(n, DENS_THREADS, 4096)), dim3(DENS_THREADS), 0, stream, x, out, n);
  return check_launch("density_sqrt_kernel");
}

}  // namespace unetdc
