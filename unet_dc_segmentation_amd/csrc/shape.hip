// Per-droplet shape and intensity integers from an int32 label map: second moments, bounding box,
// the three perimeter classes of scikit-image's perimeter(neighborhood=4) and the sum / sum of squares / minimum / maximum
// of a grey plane, per label.  Every quantity is an exact integer sum, minimum, maximum or count, accumulated with integer
// atomics only: the result does not depend on the order in which anything runs.
//
//   label_props_init     sums 0, minima INT64_MAX, maxima -1 on the [SHAPE_QUANTITIES][max_out] output
//   label_props_kernel   one wave per 64 consecutive pixels of a row (row_unit); lanes that carry the same label next to each
//                        other form a run (wave_runs, wave_ops.h), and only its head lane issues global atomics:
//                          coordinates  a run is the pixels x0 .. x0 + n - 1 of row y, so n, sum x and sum x^2 are closed
//                                       forms of (x0, n): no cross-lane traffic at all, min_x = x0, max_x = x0 + n - 1
//                          perimeter    one ballot per class, popcount under the run's lane mask
//                          grey         segmented suffix reductions (run_sum, run_min, run_max)
//                        A pixel's perimeter code needs the labels within two pixels of it.  They are read straight from
//                        the label map (5.8 MB at 1040 x 1388: it stays in L2 / the Infinity Cache between the rows),
//                        in two steps: the 4 neighbours decide whether the pixel is a border pixel at all; only border
//                        pixels read the other 16 labels of the radius-2 diamond.  Background pixels, the majority, cost the
//                        one coalesced load of their own label.
#include "kernels.h"
#include "wave_ops.h"

namespace unetdc {

enum { Q_SYY = 0, Q_SXX, Q_SXY, Q_MINY, Q_MINX, Q_MAXY, Q_MAXX, Q_P1, Q_P2, Q_P3, Q_SG, Q_SGG, Q_MING, Q_MAXG };
static_assert(Q_MAXG + 1 == SHAPE_QUANTITIES, "shape quantities");

constexpr long long SHAPE_MIN_INIT = 0x7fffffffffffffffll;

__global__ void label_props_init_kernel(long long* __restrict__ out, int max_out) {
  const long n = (long)SHAPE_QUANTITIES * max_out;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i / max_out);
    out[i] = (q == Q_MINY || q == Q_MINX || q == Q_MING) ? SHAPE_MIN_INIT : (q == Q_MAXY || q == Q_MAXX || q == Q_MAXG) ? -1ll : 0ll;
  }
}

// perimeter code -> class: bit `code` of the class's mask (codes stay below 1 + 4 * 2 + 4 * 10 = 49)
constexpr unsigned long long PERIM_CLASS1 = (1ull << 5) | (1ull << 7) | (1ull << 15) | (1ull << 17) | (1ull << 25) | (1ull << 27);
constexpr unsigned long long PERIM_CLASS2 = (1ull << 21) | (1ull << 33);
constexpr unsigned long long PERIM_CLASS3 = (1ull << 13) | (1ull << 23);

// 0 for a pixel that is not a border pixel of its label k (k > 0), else 1 + 2 * (border 4-neighbours of label k) +
// 10 * (border diagonal neighbours of label k).  Pixels outside the image carry no label.
__device__ __forceinline__ int perimeter_code(const int* __restrict__ label, int h, int w, int y, int x, int k) {
  const long i = (long)y * w + x;
  const bool up = y > 0 && label[i - w] == k, down = y + 1 < h && label[i + w] == k;
  const bool left = x > 0 && label[i - 1] == k, right = x + 1 < w && label[i + 1] == k;
  if (up && down && left && right) return 0;
  // bit (dy + 2) * 5 + (dx + 2): the pixel at (y + dy, x + dx) has label k; the four corners of the 5 x 5 square are not needed
  unsigned m = 1u << 12;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if ((dy == 0 && dx == 0) || (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx) > 3) continue;
      const int yy = y + dy, xx = x + dx;
      const bool same = yy >= 0 && yy < h && xx >= 0 && xx < w && label[(long)yy * w + xx] == k;
      m |= (same ? 1u : 0u) << ((dy + 2) * 5 + dx + 2);
    }
  }
  int code = 1;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const int b = (dy + 2) * 5 + dx + 2;
      const unsigned cross = (1u << (b - 5)) | (1u << (b + 5)) | (1u << (b - 1)) | (1u << (b + 1));
      const bool border = ((m >> b) & 1u) && (m & cross) != cross;
      code += border ? (dy != 0 && dx != 0 ? 10 : 2) : 0;
    }
  }
  return code;
}

__global__ __launch_bounds__(256) void label_props_kernel(const int* __restrict__ label, const unsigned char* __restrict__ gray,
                                                          int h, int w, long long* __restrict__ out, int max_out) {
  const int lane = threadIdx.x & 63;
  const int chunks = (w + 63) >> 6;
  const long units = (long)h * chunks;
  const long stride = (long)gridDim.x * 4;
  for (long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += stride) {   // uniform within a wave
    const auto [y, x, in, i] = row_unit(u, chunks, w, lane);
    int k = in ? label[i] : 0;
    if (k < 0 || k > max_out) k = 0;                        // labels past the capacity are skipped, never written
    if (__ballot(k > 0) == 0ull) continue;                  // wave-uniform: nothing but background here
    const WaveRuns r = wave_runs(k, lane);
    const int code = k > 0 ? perimeter_code(label, h, w, y, x, k) : 0;
    const unsigned long long c1 = __ballot((PERIM_CLASS1 >> code) & 1ull), c2 = __ballot((PERIM_CLASS2 >> code) & 1ull),
                             c3 = __ballot((PERIM_CLASS3 >> code) & 1ull);
    int sg = 0, sgg = 0, gmin = 0, gmax = 0;
    if (gray) {                                             // uniform
      const int g = in ? (int)gray[i] : 0;
      sg = run_sum(g, r, lane), sgg = run_sum(g * g, r, lane);     // 64 * 255^2 < 2^23
      gmin = run_min(g, r, lane), gmax = run_max(g, r, lane);
    }
    if (k > 0 && r.head) {
      const unsigned long long run = run_mask(r, lane);
      const long long n = r.len, x0 = x, yl = y;
      const long long sx = n * x0 + n * (n - 1) / 2;
      const long long sxx = n * x0 * x0 + x0 * n * (n - 1) + (n - 1) * n * (2 * n - 1) / 6;
      long long* o = out + (k - 1);
      const long q = max_out;
      atomic_add64(o + Q_SYY * q, yl * yl * n);
      atomic_add64(o + Q_SXX * q, sxx);
      atomic_add64(o + Q_SXY * q, yl * sx);
      atomicMin(o + Q_MINY * q, yl);
      atomicMax(o + Q_MAXY * q, yl);
      atomicMin(o + Q_MINX * q, x0);
      atomicMax(o + Q_MAXX * q, x0 + n - 1);
      const int p1 = __popcll(c1 & run), p2 = __popcll(c2 & run), p3 = __popcll(c3 & run);
      if (p1) atomic_add64(o + Q_P1 * q, p1);
      if (p2) atomic_add64(o + Q_P2 * q, p2);
      if (p3) atomic_add64(o + Q_P3 * q, p3);
      if (gray) {
        atomic_add64(o + Q_SG * q, sg);
        atomic_add64(o + Q_SGG * q, sgg);
        atomicMin(o + Q_MING * q, (long long)gmin);
        atomicMax(o + Q_MAXG * q, (long long)gmax);
      }
    }
  }
}

int launch_label_props(const int* label, const unsigned char* gray, int h, int w, long long* out, int max_out,
                       hipStream_t stream) {
  UNETDC_REQUIRE(label && (out || max_out == 0), "label_props: null pointer");
  UNETDC_REQUIRE(h > 0 && w > 0 && h <= 16384 && w <= 16384 && (long)h * w < (1L << 30) && max_out >= 0,
                 "label_props: bad geometry (sides 1..16384)");
  if (max_out == 0) return UNETDC_OK;
  long ni = ((long)SHAPE_QUANTITIES * max_out + 255) / 256;
  hipLaunchKernelGGL(label_props_init_kernel, dim3((unsigned)(ni > 1024 ? 1024 : ni)), dim3(256), 0, stream, out, max_out);
  long nb = ((long)h * ((w + 63) / 64) + 3) / 4;
  hipLaunchKernelGGL(label_props_kernel, dim3((unsigned)(nb > 8192 ? 8192 : nb)), dim3(256), 0, stream, label, gray, h, w, out,
                     max_out);
  return check_launch("label_props kernels");
}

}  // namespace unetdc
