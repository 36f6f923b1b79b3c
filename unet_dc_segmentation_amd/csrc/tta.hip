// Test-time augmentation over the dihedral group D4: the flipped and rotated copies of a batch of square
// planes, and the mean of the network's outputs on them, each mapped back first.  The rule (variants, their order, the order of
// the fp32 operations) is stated once in utils/tta.py; expand_numpy / mean_numpy there are these two kernels on the host.
//
//   variant v in 0..7: hflip = v & 4, k = v & 3; variant(P)[y][x] = P[aug_source(y, x, S, S, hflip ? AUG_HFLIP : 0, k)], that is
//            np.rot90(P[:, ::-1] if hflip else P, k).  nvar in {1, 2, 4, 8} takes the ordered lists [0], [0, 4], [0, 4, 2, 6], [0..7].
//   expand   out[b * nvar + i][c] = variant list[i] of x[b][c]: a permutation, bit-exact.
//   mean     out[b][y][x] = (q_0 + q_1 + ... ) / float(nvar) in list order, q_i[y][x] = p[b * nvar + i][aug_dest(y, x, ...)]: the
//            item mapped back through the inverse of its variant; every add rounded in fp32, one IEEE division.
//
// Every element of D4 maps an aligned 16 x 16 block of a plane onto an aligned 16 x 16 block, and acts inside the block as it acts
// on the plane.  A wave owns one block: its 64 lanes read the source block by rows, 16 bytes each (a row of a block is one
// 64-byte run), park it in LDS, pick their four destination pixels from the permuted positions and write the destination block by
// rows, 16 bytes each -- for the odd k too, where a per-thread gather would walk down columns.  Both kernels are memory-bound:
// the expand moves 4 bytes in and 4 out per output element, the mean 4 * nvar in and 4 out per output pixel.
//   mean_env the mean, and from the same LDS tile in the same trip lo / hi = the minimum / maximum over the mapped-back items
//            (DESIGN.md section 23): 4 * nvar bytes in and 12 out per pixel, where a separate pass would read the items twice.
#include "gather_index.h"
#include "kernels.h"

namespace unetdc {

constexpr int TTA_THREADS = 256, TTA_WAVES = TTA_THREADS / 64;   // a wave per 16 x 16 block, four blocks per workgroup and trip
constexpr int TTA_MAX_GROUPS = 2048;                             // grid cap, the rest goes through the grid-stride loop
constexpr int TTA_ROW = 20;                                      // LDS row stride in dwords: rows stay 16-byte aligned
constexpr int TTA_MIN_S = 16, TTA_MAX_S = 4096, TTA_MAX_N = 4096;

// the i-th variant of the ordered list of nvar variants
__device__ __forceinline__ int tta_variant(int nvar, int i) {
  return nvar == 8 ? i : nvar == 4 ? ((i & 1) << 2) | (i & 2) : i << 2;      // [0..7], [0, 4, 2, 6], [0, 4] / [0]
}

__global__ __launch_bounds__(TTA_THREADS) void dihedral_expand_kernel(const float* __restrict__ x, int cn, int S, int nvar,
                                                                      float* __restrict__ out, long nblocks) {
  __shared__ __attribute__((aligned(16))) unsigned int tile[TTA_WAVES][16 * TTA_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane >> 2, q4 = (lane & 3) * 4;
  const int nb = S / 16;
  const long plane = (long)S * S, ntrips = (nblocks + TTA_WAVES - 1) / TTA_WAVES;
  for (long trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {       // the same trips for every wave of the workgroup
    const long w = trip * TTA_WAVES + wave;
    const bool live = w < nblocks;
    const int bx = (int)(w % nb), by = (int)((w / nb) % nb);
    const long pc = w / ((long)nb * nb);                                  // output plane: item * cn + channel
    const int c = (int)(pc % cn);
    const long item = pc / cn, b = item / nvar;
    const int v = tta_variant(nvar, (int)(item % nvar)), flags = (v & 4) ? AUG_HFLIP : 0, k = v & 3;
    if (live) {
      int sy, sx;
      aug_source(16 * by, 16 * bx, S, S, flags, k, sy, sx);               // any pixel of the block names its source block
      const float* src = x + (b * cn + c) * plane + (long)((sy & ~15) + r) * S + (sx & ~15) + q4;
      st16(&tile[wave][r * TTA_ROW + q4], ld16(src));
    }
    __syncthreads();
    if (live) {
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int ly, lx;
        aug_source(r, q4 + e, 16, 16, flags, k, ly, lx);
        o[e] = tile[wave][ly * TTA_ROW + lx];
      }
      st16(out + pc * plane + (long)(16 * by + r) * S + 16 * bx + q4, o);
    }
    __syncthreads();                                                      // the tile is free for the next trip
  }
}

// The body of both mean kernels: the NVAR mapped-back items of a block through LDS, their mean in list order, and with ENV the
// per-pixel minimum and maximum of the same LDS tile (fminf / fmaxf), each output written with the same 16-byte row stores.
template <int NVAR, bool ENV>
__device__ __forceinline__ void dihedral_mean_body(unsigned int (&tile)[TTA_WAVES][NVAR][16 * TTA_ROW], const float* __restrict__ p,
                                                   int S, float* __restrict__ out, float* __restrict__ out_lo,
                                                   float* __restrict__ out_hi, long nblocks) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane >> 2, q4 = (lane & 3) * 4;
  const int nb = S / 16;
  const long plane = (long)S * S, ntrips = (nblocks + TTA_WAVES - 1) / TTA_WAVES;
  for (long trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
    const long w = trip * TTA_WAVES + wave;
    const bool live = w < nblocks;
    const int bx = (int)(w % nb), by = (int)((w / nb) % nb);
    const long b = w / ((long)nb * nb);
    if (live) {
#pragma unroll
      for (int i = 0; i < NVAR; ++i) {
        const int v = tta_variant(NVAR, i);
        int dy, dx;
        aug_dest(16 * by, 16 * bx, S, S, (v & 4) ? AUG_HFLIP : 0, v & 3, dy, dx);
        const float* src = p + (b * NVAR + i) * plane + (long)((dy & ~15) + r) * S + (dx & ~15) + q4;
        st16(&tile[wave][i][r * TTA_ROW + q4], ld16(src));
      }
    }
    __syncthreads();
    if (live) {
      float acc[4], lo[4], hi[4];
#pragma unroll
      for (int i = 0; i < NVAR; ++i) {
        const int v = tta_variant(NVAR, i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int ly, lx;
          aug_dest(r, q4 + e, 16, 16, (v & 4) ? AUG_HFLIP : 0, v & 3, ly, lx);
          const float qv = bits_f32(tile[wave][i][ly * TTA_ROW + lx]);
          acc[e] = i == 0 ? qv : acc[e] + qv;                             // list order, every add rounded
          if (ENV) {
            lo[e] = i == 0 ? qv : fminf(lo[e], qv);
            hi[e] = i == 0 ? qv : fmaxf(hi[e], qv);
          }
        }
      }
      const long at = b * plane + (long)(16 * by + r) * S + 16 * bx + q4;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f32_bits(acc[e] / (float)NVAR);
      st16(out + at, o);
      if (ENV) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f32_bits(lo[e]);
        st16(out_lo + at, o);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f32_bits(hi[e]);
        st16(out_hi + at, o);
      }
    }
    __syncthreads();
  }
}

template <int NVAR>
__global__ __launch_bounds__(TTA_THREADS) void dihedral_mean_kernel(const float* __restrict__ p, int S, float* __restrict__ out,
                                                                    long nblocks) {
  __shared__ __attribute__((aligned(16))) unsigned int tile[TTA_WAVES][NVAR][16 * TTA_ROW];
  dihedral_mean_body<NVAR, false>(tile, p, S, out, nullptr, nullptr, nblocks);
}

template <int NVAR>
__global__ __launch_bounds__(TTA_THREADS) void dihedral_mean_env_kernel(const float* __restrict__ p, int S, float* __restrict__ out,
                                                                        float* __restrict__ out_lo, float* __restrict__ out_hi,
                                                                        long nblocks) {
  __shared__ __attribute__((aligned(16))) unsigned int tile[TTA_WAVES][NVAR][16 * TTA_ROW];
  dihedral_mean_body<NVAR, true>(tile, p, S, out, out_lo, out_hi, nblocks);
}

static int tta_groups(long nblocks) {
  const long ng = (nblocks + TTA_WAVES - 1) / TTA_WAVES;
  return (int)(ng > TTA_MAX_GROUPS ? TTA_MAX_GROUPS : ng);
}

static bool tta_overlap(const void* a, long abytes, const void* b, long bbytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// the checks both entry points share; `what` names the caller in the message
static int tta_check(const char* what, const void* in, const void* out, int n, int c, int s, int nvar) {
  UNETDC_REQUIRE(in && out, "%s: null pointer", what);
  UNETDC_REQUIRE(s % 16 == 0 && s >= TTA_MIN_S && s <= TTA_MAX_S, "%s: plane size %d outside the limits (a multiple of 16 in %d..%d)",
                 what, s, TTA_MIN_S, TTA_MAX_S);
  UNETDC_REQUIRE(n >= 1 && n <= TTA_MAX_N && c >= 1 && c <= 4, "%s: bad geometry, %d images of %d channels (1..%d images, 1..4 channels)",
                 what, n, c, TTA_MAX_N);
  UNETDC_REQUIRE(nvar == 1 || nvar == 2 || nvar == 4 || nvar == 8, "%s: %d variants, not one of 1, 2, 4, 8", what, nvar);
  UNETDC_REQUIRE(reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
                 "%s: both buffers must be 16-byte aligned", what);
  return UNETDC_OK;
}

int launch_dihedral_expand(const float* x, int n, int c, int s, int nvar, float* out, hipStream_t stream) {
  if (int rc = tta_check("dihedral_expand", x, out, n, c, s, nvar)) return rc;
  const long in_elems = (long)n * c * s * s;
  UNETDC_REQUIRE(!tta_overlap(x, in_elems * 4, out, in_elems * nvar * 4), "dihedral_expand: out must not overlap the input");
  const long nblocks = in_elems * nvar / 256;
  hipLaunchKernelGGL(dihedral_expand_kernel, dim3(tta_groups(nblocks)), dim3(TTA_THREADS), 0, stream, x, c, s, nvar, out, nblocks);
  return check_launch("dihedral_expand_kernel");
}

int launch_dihedral_mean(const float* p, int n, int s, int nvar, float* out, hipStream_t stream) {
  if (int rc = tta_check("dihedral_mean", p, out, n, 1, s, nvar)) return rc;
  const long out_elems = (long)n * s * s;
  UNETDC_REQUIRE(!tta_overlap(p, out_elems * nvar * 4, out, out_elems * 4), "dihedral_mean: out must not overlap the input");
  const long nblocks = out_elems / 256;
  const dim3 grid(tta_groups(nblocks)), block(TTA_THREADS);
  switch (nvar) {
    case 1: hipLaunchKernelGGL(dihedral_mean_kernel<1>, grid, block, 0, stream, p, s, out, nblocks); break;
    case 2: hipLaunchKernelGGL(dihedral_mean_kernel<2>, grid, block, 0, stream, p, s, out, nblocks); break;
    case 4: hipLaunchKernelGGL(dihedral_mean_kernel<4>, grid, block, 0, stream, p, s, out, nblocks); break;
    default: hipLaunchKernelGGL(dihedral_mean_kernel<8>, grid, block, 0, stream, p, s, out, nblocks); break;
  }
  return check_launch("dihedral_mean_kernel");
}

int launch_dihedral_mean_env(const float* p, int n, int s, int nvar, float* out_mean, float* out_lo, float* out_hi,
                             hipStream_t stream) {
  if (int rc = tta_check("dihedral_mean_env", p, out_mean, n, 1, s, nvar)) return rc;
  UNETDC_REQUIRE(out_lo && out_hi, "dihedral_mean_env: null pointer");
  UNETDC_REQUIRE(reinterpret_cast<uintptr_t>(out_lo) % 16 == 0 && reinterpret_cast<uintptr_t>(out_hi) % 16 == 0,
                 "dihedral_mean_env: every buffer must be 16-byte aligned");
  const long out_elems = (long)n * s * s;
  float* const outs[3] = {out_mean, out_lo, out_hi};
  for (int a = 0; a < 3; ++a) {
    UNETDC_REQUIRE(!tta_overlap(p, out_elems * nvar * 4, outs[a], out_elems * 4), "dihedral_mean_env: no output may overlap the input");
    for (int b = a + 1; b < 3; ++b)
      UNETDC_REQUIRE(!tta_overlap(outs[a], out_elems * 4, outs[b], out_elems * 4), "dihedral_mean_env: the outputs must not overlap");
  }
  const long nblocks = out_elems / 256;
  const dim3 grid(tta_groups(nblocks)), block(TTA_THREADS);
  switch (nvar) {
    case 1: hipLaunchKernelGGL(dihedral_mean_env_kernel<1>, grid, block, 0, stream, p, s, out_mean, out_lo, out_hi, nblocks); break;
    case 2: hipLaunchKernelGGL(dihedral_mean_env_kernel<2>, grid, block, 0, stream, p, s, out_mean, out_lo, out_hi, nblocks); break;
    case 4: hipLaunchKernelGGL(dihedral_mean_env_kernel<4>, grid, block, 0, stream, p, s, out_mean, out_lo, out_hi, nblocks); break;
    default: hipLaunchKernelGGL(dihedral_mean_env_kernel<8>, grid, block, 0, stream, p, s, out_mean, out_lo, out_hi, nblocks); break;
  }
  return check_launch("dihedral_mean_env_kernel");
}

}  // namespace unetdc
