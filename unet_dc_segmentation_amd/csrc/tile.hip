// Tiled inference at native resolution: cut an image into overlapping network-size tiles and blend the
// tile probabilities back into one map of the image's size.  The rules (tile plan, reflect-101 fold, blend weights, order of
// the fp32 operations) are stated once in utils/tiling.py; gather_numpy / blend_numpy there are these two kernels on the host.
//
//   gather   tiles[t][c][y][x] = float(src[fold(yo[ty] + y, H)][fold(xo[tx] + x, W)][c]) / 255.0f for the tile numbers
//            t0 .. t0 + count - 1 of the plan, tile number = ty * nx + tx.  A thread makes 4 consecutive x of every channel:
//            it reads its 4 * C source bytes once and issues one 16-byte store per channel plane.  The fold makes every read
//            land inside the image WHATEVER the origin arrays hold (they live on the device and cannot be checked here).
//   blend    out[y][x] = sum(wy wx p) / sum(wy wx) over the tiles that cover (y, x), w(i) = min(i + 1, T - i, max(O, 1)) at
//            the tile-local index i.  Gather form: a thread owns one output pixel, walks the origin lists in tile order, and
//            reads tile (ty, tx) only where 0 <= y - yo[ty] < T and 0 <= x - xo[tx] < T: inside the tile for any origins, and
//            never in the folded part of a tile of an image smaller than T.  Product and sum are rounded separately
//            (fp contraction off: no fused multiply-add), one IEEE division at the end: blend_numpy bit for bit, no atomics,
//            nothing depends on an order of arrival.
// Both are memory-bound: the gather writes 4 * C * T * T bytes per tile against C * T * T bytes read, the blend reads 4 bytes per
// covering tile and pixel and writes 4.
#include "gather_index.h"
#include "kernels.h"

namespace unetdc {

constexpr int TILE_THREADS = 256;
constexpr int TILE_MAX_GROUPS = 2048;               // grid cap, the rest of the work goes through the grid-stride loops
constexpr int TILE_MIN_T = 16, TILE_MAX_T = 4096;   // the kernels' own limits; the plan of utils/tiling.py starts at 32
constexpr int TILE_MAX_SIDE = 16384;
constexpr int TILE_MAX_PER_AXIS = 1024;             // tiles per axis: tile numbers and tile offsets stay far below 2^31 / 2^63

// tile_fold (reflect-101 of any int coordinate into 0..dim-1): gather_index.h

__global__ __launch_bounds__(TILE_THREADS) void tile_gather_kernel(const unsigned char* __restrict__ src, int H, int W, int cn,
                                                                   float* __restrict__ dst, int T, const int* __restrict__ yo,
                                                                   const int* __restrict__ xo, int nx, int t0, long ngroups) {
  const int gpr = T / 4;                            // groups of 4 pixels per tile row
  const long plane = (long)T * T;
  for (long g = (long)blockIdx.x * TILE_THREADS + threadIdx.x; g < ngroups; g += (long)gridDim.x * TILE_THREADS) {
    const int xg = (int)(g % gpr);
    const long r = g / gpr;
    const int y = (int)(r % T), t = (int)(r / T);
    const int tn = t0 + t, ty = tn / nx, tx = tn - ty * nx;
    const int sy = tile_fold(yo[ty] + y, H), x0 = xo[tx] + 4 * xg;
    const unsigned char* row = src + (long)sy * W * cn;
    int sx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sx[j] = tile_fold(x0 + j, W) * cn;
    float* o = dst + (long)t * cn * plane + (long)y * T + 4 * xg;
    for (int c = 0; c < cn; ++c) {
      u32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = f32_bits((float)row[sx[j] + c] / 255.0f);
      st16(o + c * plane, v);
    }
  }
}

__global__ __launch_bounds__(TILE_THREADS) void tile_blend_kernel(const float* __restrict__ tiles, int T, int ramp,
                                                                  const int* __restrict__ yo, int ny, const int* __restrict__ xo,
                                                                  int nx, float* __restrict__ out, int W, long npix) {
#pragma clang fp contract(off)                     // plain operators under this pragma: hipcc fuses __fadd_rn(__fmul_rn()) into v_fmac_f32
  const long plane = (long)T * T;
  for (long i = (long)blockIdx.x * TILE_THREADS + threadIdx.x; i < npix; i += (long)gridDim.x * TILE_THREADS) {
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    float num = 0.0f, den = 0.0f;
    for (int ty = 0; ty < ny; ++ty) {
      const int ly = y - yo[ty];
      if ((unsigned)ly >= (unsigned)T) continue;
      int wy = ly + 1 < T - ly ? ly + 1 : T - ly;
      wy = wy < ramp ? wy : ramp;
      const float* trow = tiles + (long)ty * nx * plane + (long)ly * T;
      for (int tx = 0; tx < nx; ++tx) {
        const int lx = x - xo[tx];
        if ((unsigned)lx >= (unsigned)T) continue;
        int wx = lx + 1 < T - lx ? lx + 1 : T - lx;
        wx = wx < ramp ? wx : ramp;
        const float wf = (float)(wy * wx);          // <= (T / 2)^2 <= 2^22: exact
        const float prod = wf * trow[tx * plane + lx];
        num = num + prod;
        den = den + wf;
      }
    }
    out[i] = num / den;                             // a pixel no tile covers (origins that are not a plan) gets 0 / 0 = NaN
  }
}

static int tile_groups(long n) {
  const long nb = (n + TILE_THREADS - 1) / TILE_THREADS;
  return (int)(nb > TILE_MAX_GROUPS ? TILE_MAX_GROUPS : nb < 1 ? 1 : nb);
}

int launch_tile_gather(const unsigned char* src, int h, int w, int cn, float* tiles, int t, const int* yo, int ny, const int* xo,
                       int nx, int t0, int count, hipStream_t stream) {
  UNETDC_REQUIRE(src && tiles && yo && xo, "tile_gather: null pointer");
  UNETDC_REQUIRE(h >= 1 && w >= 1 && h <= TILE_MAX_SIDE && w <= TILE_MAX_SIDE && cn >= 1 && cn <= 4,
                 "tile_gather: bad geometry %d x %d x %d (sides 1..%d, channels 1..4)", h, w, cn, TILE_MAX_SIDE);
  UNETDC_REQUIRE(t % 16 == 0 && t >= TILE_MIN_T && t <= TILE_MAX_T, "tile_gather: tile size %d outside the limits (a multiple of 16 in %d..%d)",
                 t, TILE_MIN_T, TILE_MAX_T);
  UNETDC_REQUIRE(ny >= 1 && nx >= 1 && ny <= TILE_MAX_PER_AXIS && nx <= TILE_MAX_PER_AXIS,
                 "tile_gather: bad geometry of the plan, %d x %d tiles (1..%d per axis)", ny, nx, TILE_MAX_PER_AXIS);
  UNETDC_REQUIRE(t0 >= 0 && count >= 1 && (long)t0 + count <= (long)ny * nx,
                 "tile_gather: tiles %d .. %d + %d outside the limits of a plan of %d tiles", t0, t0, count, ny * nx);
  UNETDC_REQUIRE(reinterpret_cast<uintptr_t>(tiles) % 16 == 0, "tile_gather: the tile buffer must be 16-byte aligned");
  const long ngroups = (long)count * t * (t / 4);
  hipLaunchKernelGGL(tile_gather_kernel, dim3(tile_groups(ngroups)), dim3(TILE_THREADS), 0, stream, src, h, w, cn, tiles, t, yo, xo,
                     nx, t0, ngroups);
  return check_launch("tile_gather_kernel");
}

int launch_tile_blend(const float* tiles, int t, int overlap, const int* yo, int ny, const int* xo, int nx, float* out, int h,
                      int w, hipStream_t stream) {
  UNETDC_REQUIRE(tiles && yo && xo && out, "tile_blend: null pointer");
  UNETDC_REQUIRE(h >= 1 && w >= 1 && h <= TILE_MAX_SIDE && w <= TILE_MAX_SIDE, "tile_blend: bad geometry %d x %d (sides 1..%d)", h, w,
                 TILE_MAX_SIDE);
  UNETDC_REQUIRE(t % 16 == 0 && t >= TILE_MIN_T && t <= TILE_MAX_T, "tile_blend: tile size %d outside the limits (a multiple of 16 in %d..%d)",
                 t, TILE_MIN_T, TILE_MAX_T);
  UNETDC_REQUIRE(overlap >= 0 && 2 * overlap <= t, "tile_blend: overlap %d outside the limits 0..%d (half the tile size)", overlap, t / 2);
  UNETDC_REQUIRE(ny >= 1 && nx >= 1 && ny <= TILE_MAX_PER_AXIS && nx <= TILE_MAX_PER_AXIS,
                 "tile_blend: bad geometry of the plan, %d x %d tiles (1..%d per axis)", ny, nx, TILE_MAX_PER_AXIS);
  const long npix = (long)h * w;
  hipLaunchKernelGGL(tile_blend_kernel, dim3(tile_groups(npix)), dim3(TILE_THREADS), 0, stream, tiles, t, overlap > 1 ? overlap : 1, yo,
                     ny, xo, nx, out, w, npix);
  return check_launch("tile_blend_kernel");
}

}  // namespace unetdc
