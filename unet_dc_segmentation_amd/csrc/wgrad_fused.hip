// Tap-fused weight gradient of the dilated 3x3 convolutions (64x64 channel tiles, d <= 8).
//
//   dW[t][co][ci] = sum_p dY[p][co] * X[p + off_t][ci]                (autograd of nn.Conv2d,
//                                                                     models/model_2.py:41-51)
// The per-tap kernel (wgrad_dma.hip) re-stages dY and X for each of the 9 taps and, on a 64x64 tile,
// gets only 8 MFMAs per wave between barriers: it ran at ~370 TFLOP/s on enc1/dec1.  Here one
// workgroup walks down a vertical strip of the image (SEG pixels wide).  Per image row it stages
//   * the dY row segment            [SEG pixels][64 co]
//   * three X row segments y-d,y,y+d [SEG + 2d (padded to SEG+16) pixels][64 ci]  (zero outside)
// by LDS-DMA and accumulates ALL NINE taps from them: tap (ky,kx) reads X segment ky at pixel rows
// shifted by kx*d.  9x the MFMA work per staged byte and per barrier.
// fp32 (wgrad_fused_kernel, wgrad_ring_kernel): 2x2 quadrants of the 64x64 (co x ci) tile per wave,
// 9 accumulators (one per tap) each, fragments by scalar reads.  bf16 (the tap-split kernels): wave
// roles below, fragments via ds_read_b64_tr_b16 on the [pixel][channel] image (wgrad_frag.h).
// Strips x y-ranges give the K split; partial slabs are reduced by wgrad_reduce_kernel (deterministic).
#include <stdio.h>
#include <stdlib.h>

#include "kernels.h"
#include "lds_dma.h"
#include "wgrad_frag.h"

namespace unetdc {

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
constexpr unsigned FOOB = 0x80000000u;

struct WgradFusedParams {
  const void* dy;   // [P][lddy], channels -> i
  const void* x;    // [P][ldx],  channels -> j
  float* part;      // [units][9][CI][CJ]
  int N, H, W, CI, CJ, lddy, ldx, d;
  int ysplit, rows_per_unit, itiles, jtiles;
  int imgs_per_unit;   // tap-split ring kernel with ysplit == 1: a workgroup walks this many images of its segment in turn
  int half_lds;        // paired form (HV = 2): LDS bytes of one half's ring
  // input normalisation ("bnin", tap-split ring kernel): x is the RAW conv output of the producing stage; every X row is
  // normalised in LDS, relu(in_scale * x + in_shift) rounded through bf16, once, when it has landed
  const float* in_scale;
  const float* in_shift;
};

#ifdef UNETDC_WGRAD_STAMPS
// DIAGNOSTIC BUILD ONLY (tools/probes/wgrad_stamps.sh; never part of libunetdc_hip.so): per wave, the shader-clock cycles of a
// step spent (0) in the counted vmcnt wait, (1) at the workgroup barrier, (2) from the barrier to the first MFMA (first fragment
// reads + DMA issue), (3) in the item loop, summed over the steps; [4] = steps.  Written once at the end, read by nothing.
__device__ unsigned long long g_wgrad_stamps[512][8][5];
extern "C" int unetdc_dbg_wgrad_stamps(unsigned long long* dst) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wgrad_stamps), sizeof(g_wgrad_stamps));
}
#define STAMP(var) unsigned long long var = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif

constexpr int SEG_BF16 = 64, SEG_F32 = 32;     // pixels of a strip's row segment

// fp32 (bf16 runs the tap-split kernels below)
__global__ __launch_bounds__(256, 2) void wgrad_fused_kernel(const WgradFusedParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  using T = float;
  constexpr int SEG = SEG_F32;
  constexpr int XR = SEG + 16;                         // X segment rows (x0-d .. x0+SEG-1+d, d <= 8)
  constexpr int ES = (int)sizeof(T);
  constexpr int RB = 64 * ES;                          // bytes per pixel row (64 channels)
  constexpr int CPR = RB / 16, RPI = 64 / CPR;         // lanes per row, rows per DMA instruction
  constexpr int DYI = SEG / RPI, XI = XR / RPI;        // DMA instructions: dY segment, one X segment
  constexpr int NSLOT = (DYI + 3 * XI + 3) / 4;        // per wave
  constexpr int DYB = SEG * RB, XB = XR * RB;
  constexpr int STAGE = DYB + 3 * XB;
  static_assert(SEG % RPI == 0 && XR % RPI == 0, "segment/instruction mismatch");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lds_base = lds_addr_of(smem);
  const int qi = wave >> 1, qj = wave & 1;
  // block -> (unit, it, jt); unit -> (image, x segment, y range)
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles = p.itiles * p.jtiles;
  const int unit = L / tiles, trem = L - unit * tiles;
  const int it = trem / p.jtiles, jt = trem - it * p.jtiles;
  const int i0 = it * 64, j0 = jt * 64;
  const int segs = p.W / SEG;
  const int ys = unit % p.ysplit, strip = unit / p.ysplit;
  const int n = strip / segs, x0 = (strip - n * segs) * SEG;
  const int ybeg = ys * p.rows_per_unit;
  const int yend = min(ybeg + p.rows_per_unit, p.H);

  const unsigned dybytes = (unsigned)((long)p.N * p.H * p.W * p.lddy * ES);
  const unsigned xbytes = (unsigned)((long)p.N * p.H * p.W * p.ldx * ES);
  const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.dy), 0, dybytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, xbytes, 0x00020000);

  // ---- DMA slots of this wave: slot q -> global instruction index gi = wave + 4*q --------------
  //   gi < DYI            : dY segment, instruction gi
  //   gi = DYI + ky*XI + k: X segment ky, instruction k
  const int sub = lane / CPR, pc = lane % CPR;
  unsigned colb[NSLOT];          // byte offset inside the image row (pixel * ld + channel chunk) or FOOB
#pragma unroll
  for (int q = 0; q < NSLOT; ++q) {
    const int gi = wave + 4 * q;
    if (gi < DYI) {
      const int row = gi * RPI + sub;                                  // pixel x0 + row
      const int c = Frag<T, 1>::src_chunk(row, pc);
      colb[q] = (unsigned)(((x0 + row) * p.lddy + i0) * ES + c * 16);
    } else if (gi < DYI + 3 * XI) {
      const int k = (gi - DYI) % XI;
      const int row = k * RPI + sub;                                   // pixel x0 - d + row
      const int gx = x0 - p.d + row;
      const int c = Frag<T, 1>::src_chunk(row, pc);
      colb[q] = ((unsigned)gx < (unsigned)p.W) ? (unsigned)((gx * p.ldx + j0) * ES + c * 16) : FOOB;
    } else {
      colb[q] = FOOB;
    }
  }

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  auto issue = [&](int stage, int y) {
#pragma unroll
    for (int q = 0; q < NSLOT; ++q) {
      const int gi = wave + 4 * q;                                     // wave-uniform
      if (gi < DYI) {
        const unsigned rowbase = (unsigned)((long)(n * p.H + y) * p.W * p.lddy * ES);
        lds_dma16(dyr, lds_base + stage * STAGE + gi * 1024, colb[q], rowbase);
      } else if (gi < DYI + 3 * XI) {
        const int ky = (gi - DYI) / XI, k = (gi - DYI) - ky * XI;
        const int yy = y + (ky - 1) * p.d;
        const bool yok = (unsigned)yy < (unsigned)p.H;
        const unsigned rowbase = (unsigned)((long)(n * p.H + (yok ? yy : 0)) * p.W * p.ldx * ES);
        const unsigned v = (yok && colb[q] != FOOB) ? colb[q] : FOOB;
        lds_dma16(xr, lds_base + stage * STAGE + DYB + ky * XB + k * 1024, v, rowbase);
      }
    }
  };

  const int nsteps = yend - ybeg;
  if (nsteps > 0) issue(0, ybeg);
  for (int s = 0; s < nsteps; ++s) {
    wait_vmcnt<0>();                                   // asm DMA + raw barrier: see lds_dma.h
    raw_barrier();
    if (s + 1 < nsteps) issue((s + 1) & 1, ybeg + s + 1);
    const unsigned char* sdy = smem + (s & 1) * STAGE;
    const unsigned char* sx = sdy + DYB;
#pragma unroll
    for (int k16 = 0; k16 < SEG / 16; ++k16) {
      const int r = lane & 31, h = lane >> 5;
#pragma unroll
      for (int kp = 0; kp < 8; ++kp) {
        const int krow = 16 * k16 + 2 * kp + h;
        const float fa = *reinterpret_cast<const float*>(sdy + krow * RB + (qi * 32 + r) * 4);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int ky = t / 3, kx = t - ky * 3;
          const float fb = *reinterpret_cast<const float*>(sx + ky * XB + (krow + kx * p.d) * RB + (qj * 32 + r) * 4);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[t], 0, 0, 0);
        }
      }
    }
  }

  // ---- partial slab: part[unit][t][i][j] ---------------------------------------------------------
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    float* slab = p.part + ((long)unit * 9 + t) * p.CI * p.CJ;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int i = i0 + qi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h, j = j0 + qj * 32 + r;
      slab[(long)i * p.CJ + j] = acc[t][reg];
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

// ------------------------------------------------------------------------------------------------
// Ring variant for d <= 2 (every decoder level, enc1, enc2: most of the weight-gradient time).  The bf16 form it was built
// and measured as is now the tap-split ring kernel below; in fp32 only PF = 1 at d = 1 fits (ring_lds).
//
// SQ counters of the kernel above on enc1 (64->64, 512x512): MFMA pipe busy 40 %; a step lasts ~4.8K cycles of
// which the two resident waves of a SIMD keep the MFMA pipe busy 2.3K -- the rest is the LDS-DMA of the NEXT
// step (issued one step ahead, 38 KB) not having landed.  But consecutive image rows share their X rows:
// rows y-d, y, y+d of step s are rows y+1-2d.. of later steps, so the three X segments live in a RING of
// R = 2d + PF + 1 row slots and a step only fetches ONE new X row plus the dY row (18 KB instead of 38 KB),
// PF steps ahead (PF = 2 when the ring fits 80 KB so that two workgroups still share a CU).
//   group k (the loads of step k) = dY row ybeg+k -> dY slot k % (PF+1);  X row ybeg+k+d -> X slot (k+2d) % R
//   step s: wait for group s (counted vmcnt: the younger group may stay in flight) ; barrier (everyone's
//   group s has landed AND everyone is done with step s-1, whose oldest X row / dY slot are now free) ;
//   issue group s+PF into exactly those slots ; 36 MFMAs per wave.
template <int PF>
__global__ __launch_bounds__(256, 2) void wgrad_ring_kernel(const WgradFusedParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  using T = float;
  constexpr int SEG = SEG_F32;
  constexpr int XR = SEG + 16;
  constexpr int ES = (int)sizeof(T);
  constexpr int RB = 64 * ES;
  constexpr int CPR = RB / 16, RPI = 64 / CPR;
  constexpr int DYI = SEG / RPI, XI = XR / RPI;
  constexpr int GI = DYI + XI;                         // DMA instructions of one group (whole workgroup)
  constexpr int NQ = (GI + 3) / 4;                     // slots per wave
  constexpr int DYB = SEG * RB, XB = XR * RB;
  constexpr int NDY = PF + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const xring = smem + NDY * DYB;
  const unsigned lds_base = lds_addr_of(smem);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = wave >> 1, qj = wave & 1;
  const int d = p.d, R = 2 * d + PF + 1;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles = p.itiles * p.jtiles;
  const int unit = L / tiles, trem = L - unit * tiles;
  const int it = trem / p.jtiles, jt = trem - it * p.jtiles;
  const int i0 = it * 64, j0 = jt * 64;
  const int segs = p.W / SEG;
  const int ys = unit % p.ysplit, strip = unit / p.ysplit;
  const int n = strip / segs, x0 = (strip - n * segs) * SEG;
  const int ybeg = ys * p.rows_per_unit;
  const int yend = min(ybeg + p.rows_per_unit, p.H);
  const int nsteps = yend - ybeg;

  const unsigned dybytes = (unsigned)((long)p.N * p.H * p.W * p.lddy * ES);
  const unsigned xbytes = (unsigned)((long)p.N * p.H * p.W * p.ldx * ES);
  const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.dy), 0, dybytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, xbytes, 0x00020000);

  // DMA slot q of this wave -> instruction gi = wave + 4q of a group: gi < DYI: dY row; else X row instruction gi - DYI
  const int sub = lane / CPR, pc = lane % CPR;
  unsigned colb[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int gi = wave + 4 * q;
    if (gi < DYI) {
      const int row = gi * RPI + sub;
      colb[q] = (unsigned)(((x0 + row) * p.lddy + i0) * ES + Frag<T, 1>::src_chunk(row, pc) * 16);
    } else if (gi < GI) {
      const int row = (gi - DYI) * RPI + sub;
      const int gx = x0 - d + row;
      colb[q] = ((unsigned)gx < (unsigned)p.W) ? (unsigned)((gx * p.ldx + j0) * ES + Frag<T, 1>::src_chunk(row, pc) * 16) : FOOB;
    } else {
      colb[q] = FOOB;
    }
  }
  const bool five = (wave + 4 * (NQ - 1)) < GI;          // does this wave's last slot exist? (wave-uniform)

  // X row `yy` of the image -> ring slot `slot` (zeros when the row lies outside the image)
  auto issue_x = [&](int slot, int yy) {
    const bool yok = (unsigned)yy < (unsigned)p.H;
    const unsigned rowbase = (unsigned)((long)(n * p.H + (yok ? yy : 0)) * p.W * p.ldx * ES);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int gi = wave + 4 * q;
      if (gi >= DYI && gi < GI) {
        const unsigned v = (yok && colb[q] != FOOB) ? colb[q] : FOOB;
        lds_dma16(xr, lds_base + NDY * DYB + slot * XB + (gi - DYI) * 1024, v, rowbase);
      }
    }
  };
  auto issue_dy = [&](int slot, int y) {
    const unsigned rowbase = (unsigned)((long)(n * p.H + y) * p.W * p.lddy * ES);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int gi = wave + 4 * q;
      if (gi < DYI) lds_dma16(dyr, lds_base + slot * DYB + gi * 1024, colb[q], rowbase);
    }
  };

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  // prologue: X rows ybeg-d .. ybeg+d-1 (ring rows 0 .. 2d-1), then groups 0 .. PF-1
  for (int rho = 0; rho < 2 * d; ++rho) issue_x(rho, ybeg - d + rho);
  int gslot_x = 2 * d, gslot_dy = 0;                     // slots of the next group to issue
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    if (k < nsteps) {
      issue_dy(gslot_dy, ybeg + k);
      issue_x(gslot_x, ybeg + k + d);
      gslot_dy = (gslot_dy + 1 == NDY) ? 0 : gslot_dy + 1;
      gslot_x = (gslot_x + 1 == R) ? 0 : gslot_x + 1;
    }
  }
  int sl0 = 0, sl1 = d, sl2 = 2 * d, sdy = 0;            // ring slots of rows y-d, y, y+d and the dY slot of step s
  for (int s = 0; s < nsteps; ++s) {
    if (PF == 2 && s + 1 < nsteps) {                     // the group of step s+1 may stay in flight
      if (five) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ - 1) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // Raw barrier behind the counted wait (lds_dma.h: with the builtin DMA + __syncthreads() of round 1 the binary
    // drained the VM counter twice per step -- `vmcnt(4|5) ; vmcnt(0) ; s_barrier` here and another compiler-inserted
    // `vmcnt(0)` in front of the first fragment read -- so the group issued for step s+2 never stayed in flight).
    raw_barrier();
    if (s + PF < nsteps) {
      issue_dy(gslot_dy, ybeg + s + PF);
      issue_x(gslot_x, ybeg + s + PF + d);
      gslot_dy = (gslot_dy + 1 == NDY) ? 0 : gslot_dy + 1;
      gslot_x = (gslot_x + 1 == R) ? 0 : gslot_x + 1;
    }
    const unsigned char* sdyp = smem + sdy * DYB;
    const unsigned char* sx[3] = {xring + sl0 * XB, xring + sl1 * XB, xring + sl2 * XB};
#pragma unroll
    for (int k16 = 0; k16 < SEG / 16; ++k16) {
      const int r = lane & 31, h = lane >> 5;
#pragma unroll
      for (int kp = 0; kp < 8; ++kp) {
        const int krow = 16 * k16 + 2 * kp + h;
        const float fa = *reinterpret_cast<const float*>(sdyp + krow * RB + (qi * 32 + r) * 4);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int ky = t / 3, kx = t - ky * 3;
          const float fb = *reinterpret_cast<const float*>(sx[ky] + (krow + kx * d) * RB + (qj * 32 + r) * 4);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[t], 0, 0, 0);
        }
      }
    }
    sl0 = (sl0 + 1 == R) ? 0 : sl0 + 1;
    sl1 = (sl1 + 1 == R) ? 0 : sl1 + 1;
    sl2 = (sl2 + 1 == R) ? 0 : sl2 + 1;
    sdy = (sdy + 1 == NDY) ? 0 : sdy + 1;
  }

  // ---- partial slab: part[unit][t][i][j] ---------------------------------------------------------
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    float* slab = p.part + ((long)unit * 9 + t) * p.CI * p.CJ + (long)(i0 + qi * 32 + 4 * h) * p.CJ + j0 + qj * 32 + r;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) slab[(long)((reg & 3) + 8 * (reg >> 2)) * p.CJ] = acc[t][reg];
  }
#endif  // __HIP_DEVICE_COMPILE__
}

// ------------------------------------------------------------------------------------------------
// Tap-split ring kernel (bf16): same staging as wgrad_ring_kernel, different split of the work over the four waves.
//
// SQ counters of wgrad_ring_kernel (profiles/r02_sq_baseline.json, 128->128 @ 256x256): 2.22 LDS instructions per MFMA,
// MFMA pipe busy 50 %.  With one 32x32 (co x ci) quadrant and all nine taps per wave, every MFMA needs a B fragment of
// its own (two ds_read_b64_tr_b16 = 1 KB): 10 fragments per 9 MFMAs.  Four SIMDs x 1 KB per 32-cycle MFMA is more than the
// LDS delivers, so the matrix pipe waits on fragment reads half the time.
// Here a wave owns BOTH co halves (64 co x 32 ci) and HALF of the taps: a B fragment feeds every co tile of the wave.
// The kernels run on v_mfma_f32_16x16x32_bf16: they are power bound like the convolutions (igemm_dma16.hip), and
// MI355X_MICROARCH.md measures 1.12-1.15x the FLOP/s for that shape at equal cycles per FLOP with operands re-read from
// LDS.  A wave holds 4 x 2 tiles of 16 x 16 per tap slot, 160 accumulator registers.
//   wave = (qj: ci half, tg: tap group).  A row of 64 pixels is two k32 steps; tg 0 takes taps 0..4 on the first and 0..3
//   on the second, tg 1 taps 5..8 and 4..8: nine items of 8 MFMAs each, tap 4 split over the two groups.
// The two partial sums of tap 4 are added through LDS at the end, tg 0's + tg 1's (fixed order).  Image swizzle and fragment
// addresses: wgrad_frag.h, Frag16.  (An earlier form of these wave roles ran on the 32x32x16 MFMA shape; its history is in
// docs/optimisation_log.md, round 3.)
// ------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int s16_k32(int tg, int i) { return tg == 0 ? (i < 5 ? 0 : 1) : (i < 4 ? 0 : 1); }
__host__ __device__ constexpr int s16_tap(int tg, int i) { return tg == 0 ? (i < 5 ? i : i - 5) : (i < 4 ? 5 + i : i); }

struct Split16Offs {       // per-lane byte offsets of the transposed reads at k32 step 0 (step 1: + 32 rows = 4096 bytes)
  int dy[4][2];            // [co tile][block jj]
  int x[3][2][2];          // [kx][ci tile][block jj], pixel rows shifted by kx * d
};

struct SplitAcc { f32x4 a[5][4][2]; };       // [tap slot][co tile][ci tile]

__device__ __forceinline__ void split_zero(SplitAcc& A) {
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) A.a[t][c][j][e] = 0.f;
}

// One image row of the strip.  `issue`: the row's DMA statements, placed behind the step's first fragment reads (those are in flight while the wave gets
// its DMA instructions accepted; round 4, as in igemm_lattice.hip)
template <int TG, typename Issue>
__device__ __forceinline__ void ring_split_step16(f32x4 (&acc)[5][4][2], const unsigned char* sdy, const unsigned char* sx0,
                                                  const unsigned char* sx1, const unsigned char* sx2, const Split16Offs& o,
                                                  Issue&& issue) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NI = 9;
  // A (dY) fragments: ONE set of four, refilled in place for the second k32 step -- each one right behind the two MFMAs of
  // the first step's last item that read it (an in-order wave: an issued MFMA has its operands) -- 16 registers instead of
  // 32: with a double set the kernel needs more than the 256 registers two workgroups per CU leave a wave.
  // B (X) fragments: two sets of two, item i + 1 loaded in front of the MFMAs of item i.
  bf16x8 fa[4], fb[2][2];
  auto load_a1 = [&](int k32, int c) { fa[c] = Frag16::frag_at(sdy + k32 * 4096, o.dy[c][0], o.dy[c][1]); };
  auto load_b = [&](int i) {
    const int k32 = s16_k32(TG, i), t = s16_tap(TG, i), ky = t / 3, kx = t - 3 * ky;
    const unsigned char* sx = (ky == 0 ? sx0 : (ky == 1 ? sx1 : sx2)) + k32 * 4096;
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[i & 1][j] = Frag16::frag_at(sx, o.x[kx][j][0], o.x[kx][j][1]);
  };
#pragma unroll
  for (int c = 0; c < 4; ++c) load_a1(0, c);
  load_b(0);
  issue();
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int k32 = s16_k32(TG, i);
    const bool turn = i + 1 < NI && s16_k32(TG, i + 1) != k32;      // last item of the first k32 step
    if (i + 1 < NI) load_b(i + 1);
    __builtin_amdgcn_sched_barrier(0);
    const int slot = s16_tap(TG, i) - (TG == 0 ? 0 : 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[slot][c][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[c], fb[i & 1][j], acc[slot][c][j], 0, 0, 0);
      if (turn) {
        __builtin_amdgcn_sched_barrier(0);
        load_a1(k32 + 1, c);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#endif
}

// tap 4: tg 1's half (slot 0) joins tg 0's (slot 4) through LDS (fixed order), then the partial slab part[unit][t][i][j]:
// tg 0 stores taps 0..4, tg 1 taps 5..8.  The caller guarantees that every DMA has landed and every fragment has been read.
// PAIRED FORM (HV = 2, 512 threads): the workgroup is two halves of four waves with the roles above, each half walking its
// own half of the unit's image rows through its own LDS ring; here the second half hands its accumulators to the first
// through LDS (ex: [wave of the half][register quad][lane], 144 KB of the then idle rings) and only the first half stores.
// Why: the fp32 slabs are the accumulator state of the whole chip (2 x 256 threads x 160 registers per CU = 84 MB per launch),
// written once and re-read by the reduce kernel; two K ranges that meet in LDS halve both (round 4).
template <int HV>
__device__ __forceinline__ void split_finish(SplitAcc& A, unsigned char* smem, unsigned char* smem_all, int half,
                                             const WgradFusedParams& p, int unit, int i0, int j0, int qj, int tg, int lane) {
  float* xch = reinterpret_cast<float*>(smem);             // [qj][co tile][ci tile][v][lane]: 16 KB
  __syncthreads();
  if (tg == 1) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) xch[(((qj * 4 + c) * 2 + j) * 4 + v) * 64 + lane] = A.a[0][c][j][v];
  }
  __syncthreads();
  if (tg == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) A.a[4][c][j][v] += xch[(((qj * 4 + c) * 2 + j) * 4 + v) * 64 + lane];
  }
  if (HV == 2) {
    __syncthreads();                                       // both halves are done with their tap-4 exchange areas
    f32x4* ex = reinterpret_cast<f32x4*>(smem_all) + (tg == 0 ? qj * 40 : 80 + qj * 32) * 64 + lane;
    if (half == 1) {
#pragma unroll
      for (int sl = 0; sl < 5; ++sl) {
        if (tg == 1 && sl == 0) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 2; ++j) ex[(((sl - (tg == 1 ? 1 : 0)) * 4 + c) * 2 + j) * 64] = A.a[sl][c][j];
      }
    }
    __syncthreads();
    if (half == 1) return;
#pragma unroll
    for (int sl = 0; sl < 5; ++sl) {
      if (tg == 1 && sl == 0) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 o = ex[(((sl - (tg == 1 ? 1 : 0)) * 4 + c) * 2 + j) * 64];
#pragma unroll
          for (int v = 0; v < 4; ++v) A.a[sl][c][j][v] += o[v];          // element by element: no packed-fp32 VALU (build guard)
        }
    }
  }
  // accumulator element v of a 16 x 16 tile: row (co) 4 * (lane >> 4) + v, column (ci) lane & 15
  const int col = lane & 15, rq = lane >> 4;
#pragma unroll
  for (int sl = 0; sl < 5; ++sl) {
    if (tg == 1 && sl == 0) continue;
    const int t = sl + (tg == 0 ? 0 : 4);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float* slab = p.part + ((long)unit * 9 + t) * p.CI * p.CJ + (long)(i0 + 16 * c + 4 * rq) * p.CJ + j0 + qj * 32 + 16 * j + col;
#pragma unroll
        for (int v = 0; v < 4; ++v) slab[(long)v * p.CJ] = A.a[sl][c][j][v];
      }
  }
}

__device__ __forceinline__ Split16Offs split_offsets(int lane, int qj, int d) {
  Split16Offs o;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) o.dy[c][jj] = Frag16::rd_off(lane, 16 * c, 0, jj);
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) o.x[kx][j][jj] = Frag16::rd_off(lane, qj * 32 + 16 * j, kx * d, jj);
  return o;
}

template <int PF, int TG, bool INORM, int HV>
__device__ __forceinline__ void ring_split_body(const WgradFusedParams& p) {
#if defined(__HIP_DEVICE_COMPILE__)
  using T = bf16_t;
  constexpr int SEG = SEG_BF16;
  constexpr int XR = SEG + 16;
  constexpr int ES = (int)sizeof(T);
  constexpr int RB = 64 * ES;
  constexpr int CPR = RB / 16, RPI = 64 / CPR;
  constexpr int DYI = SEG / RPI, XI = XR / RPI;
  constexpr int GI = DYI + XI;
  constexpr int NQ = (GI + 3) / 4;
  constexpr int DYB = SEG * RB, XB = XR * RB;
  constexpr int NDY = PF + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
  // paired form: tid / wave count inside the half, every LDS address is relative to the half's ring
  const int half = HV == 2 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;
  unsigned char* const smem = smem_all + half * p.half_lds;
  unsigned char* const xring = smem + NDY * DYB;
  const unsigned lds_base = lds_addr_of(smem);

  const int tid = threadIdx.x & 255, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qj = wave & 1;
  constexpr int tg = TG;
  const int d = p.d, R = 2 * d + PF + 1;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles = p.itiles * p.jtiles;
  const int unit = L / tiles, trem = L - unit * tiles;
  const int it = trem / p.jtiles, jt = trem - it * p.jtiles;
  const int i0 = it * 64, j0 = jt * 64;
  const int segs = p.W / SEG;
  const int ys = unit % p.ysplit, strip = unit / p.ysplit;
  // imgs_per_unit > 1 (only with ysplit == 1): the workgroup accumulates over several images of one segment, so a layer
  // with many channel tiles writes fewer fp32 slabs (1024 -> 512 channels at 64 x 64: 8 slabs of 18.9 MB were written and
  // re-read by the reduce kernel, and 1024 workgroups made two rounds on the chip)
  const int ipu = p.imgs_per_unit > 1 ? p.imgs_per_unit : 1;
  const int n0 = (strip / segs) * ipu, x0 = (strip - (strip / segs) * segs) * SEG;
  int n = n0;
  // paired form: the unit's rows are cut in two equal parts (the host only pairs when rows_per_unit is even and divides H:
  // both halves then run the same number of steps and meet at every workgroup barrier)
  const int rows_h = HV == 2 ? p.rows_per_unit / 2 : p.rows_per_unit;
  const int ybeg = ys * p.rows_per_unit + half * rows_h;
  const int yend = min(ybeg + rows_h, p.H);
  const int nsteps = yend - ybeg;

  const unsigned dybytes = (unsigned)((long)p.N * p.H * p.W * p.lddy * ES);
  const unsigned xbytes = (unsigned)((long)p.N * p.H * p.W * p.ldx * ES);
  const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.dy), 0, dybytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, xbytes, 0x00020000);

  const int sub = lane / CPR, pc = lane % CPR;
  unsigned colb[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int gi = wave + 4 * q;
    if (gi < DYI) {
      const int row = gi * RPI + sub;
      colb[q] = (unsigned)(((x0 + row) * p.lddy + i0) * ES + Frag16::src_chunk(row, pc) * 16);
    } else if (gi < GI) {
      const int row = (gi - DYI) * RPI + sub;
      const int gx = x0 - d + row;
      colb[q] = ((unsigned)gx < (unsigned)p.W) ? (unsigned)((gx * p.ldx + j0) * ES + Frag16::src_chunk(row, pc) * 16) : FOOB;
    } else {
      colb[q] = FOOB;
    }
  }
  const bool five = (wave + 4 * (NQ - 1)) < GI;

  auto issue_x = [&](int slot, int yy) {
    const bool yok = (unsigned)yy < (unsigned)p.H;
    const unsigned rowbase = (unsigned)((long)(n * p.H + (yok ? yy : 0)) * p.W * p.ldx * ES);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int gi = wave + 4 * q;
      if (gi >= DYI && gi < GI) {
        const unsigned v = (yok && colb[q] != FOOB) ? colb[q] : FOOB;
        lds_dma16(xr, lds_base + NDY * DYB + slot * XB + (gi - DYI) * 1024, v, rowbase);
      }
    }
  };
  auto issue_dy = [&](int slot, int y) {
    const unsigned rowbase = (unsigned)((long)(n * p.H + y) * p.W * p.lddy * ES);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int gi = wave + 4 * q;
      if (gi < DYI) lds_dma16(dyr, lds_base + slot * DYB + gi * 1024, colb[q], rowbase);
    }
  };

  SplitAcc acc;
  split_zero(acc);
  const Split16Offs offs = split_offsets(lane, qj, d);
  // INORM: the 64 (scale, shift) pairs of this workgroup's input-channel tile live in LDS behind the ring (no vector-memory
  // operation may join the hand-counted DMA queue inside the row loop); a thread owns logical chunk tid & 7 of every 32nd
  // pixel of a row.  Rows / pixels outside the image were zero-filled by the DMA and stay zero (zero padding of the
  // ACTIVATION); the result is rounded through bf16 like a stored activation: bit-identical to the two-pass form.
  float* const ncst = reinterpret_cast<float*>(xring + R * XB);              // [2][64]
  if (INORM) {
    if (tid < 128) ncst[tid] = (tid < 64 ? p.in_scale : p.in_shift)[j0 + (tid & 63)];
    __syncthreads();
  }
  auto normalise_row = [&](int slot, int yy) {
    if ((unsigned)yy >= (unsigned)p.H) return;                               // a zero row (wave-uniform condition)
    const int lc = tid & 7;
    float nsc[8], nsh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { nsc[e] = ncst[lc * 8 + e]; nsh[e] = ncst[64 + lc * 8 + e]; }
#pragma unroll
    for (int i = 0; i < (XR + 31) / 32; ++i) {
      const int px = (tid >> 3) + 32 * i;
      const int gx = x0 - d + px;
      if (px < XR && (unsigned)gx < (unsigned)p.W) {
        unsigned char* a = xring + slot * XB + px * RB + (Frag16::src_chunk(px, lc) << 4);
        float v[8];
        Chunk<bf16_t>::unpack(ld16(a), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(fmaf(v[e], nsc[e], nsh[e]), 0.f);
        st16(a, Chunk<bf16_t>::pack(v));
      }
    }
  };

#ifdef UNETDC_WGRAD_STAMPS
  unsigned long long st_sum[5] = {0, 0, 0, 0, 0}, st_t2 = 0;
  const unsigned long long st_kernel0 = __builtin_amdgcn_s_memtime();
#endif
  for (int img = 0; img < ipu && n0 + img < p.N; ++img) {
  n = n0 + img;
  if (img > 0) raw_barrier();                            // the previous image's last fragments have been read by every wave
  for (int rho = 0; rho < 2 * d; ++rho) issue_x(rho, ybeg - d + rho);
  int gslot_x = 2 * d, gslot_dy = 0;
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    if (k < nsteps) {
      issue_dy(gslot_dy, ybeg + k);
      issue_x(gslot_x, ybeg + k + d);
      gslot_dy = (gslot_dy + 1 == NDY) ? 0 : gslot_dy + 1;
      gslot_x = (gslot_x + 1 == R) ? 0 : gslot_x + 1;
    }
  }
  int sl0 = 0, sl1 = d, sl2 = 2 * d, sdy = 0;
  for (int s = 0; s < nsteps; ++s) {
#ifdef UNETDC_WGRAD_STAMPS
    STAMP(t0);
#endif
    if (PF == 2 && s + 1 < nsteps) {                     // the group of step s+1 may stay in flight (in-order retirement)
      if (five) wait_vmcnt<NQ>();
      else wait_vmcnt<NQ - 1>();
    } else {
      wait_vmcnt<0>();
    }
#ifdef UNETDC_WGRAD_STAMPS
    STAMP(t1);
#endif
    raw_barrier();
#ifdef UNETDC_WGRAD_STAMPS
    STAMP(t2);
    st_sum[0] += t1 - t0; st_sum[1] += t2 - t1; st_t2 = t2;
#endif
    if (INORM) {
      // the X rows that have landed with this step and were not normalised yet: at the first step of an image the 2d rows
      // issued up front and the row of group 0, afterwards the one new row y + d (ring slot sl2)
      if (s == 0) {
        for (int rho = 0; rho < 2 * d; ++rho) normalise_row(rho, ybeg - d + rho);
      }
      normalise_row(sl2, ybeg + s + d);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      raw_barrier();
    }
    auto issue_row = [&]() {
      if (s + PF < nsteps) {
        issue_dy(gslot_dy, ybeg + s + PF);
        issue_x(gslot_x, ybeg + s + PF + d);
        gslot_dy = (gslot_dy + 1 == NDY) ? 0 : gslot_dy + 1;
        gslot_x = (gslot_x + 1 == R) ? 0 : gslot_x + 1;
      }
    };
    const unsigned char* sdyp = smem + sdy * DYB;
    // (the input-normalising form keeps its DMA statements in front: behind the reads it measured 221.7 vs 214.5 us)
    if (INORM) {
      issue_row();
      ring_split_step16<TG>(acc.a, sdyp, xring + sl0 * XB, xring + sl1 * XB, xring + sl2 * XB, offs, []() {});
    } else {
      ring_split_step16<TG>(acc.a, sdyp, xring + sl0 * XB, xring + sl1 * XB, xring + sl2 * XB, offs, issue_row);
    }
#ifdef UNETDC_WGRAD_STAMPS
    {
      STAMP(t4);
      st_sum[3] += t4 - st_t2;                            // barrier -> end of the step (first reads + items)
      st_sum[4] += 1;
    }
#endif
    sl0 = (sl0 + 1 == R) ? 0 : sl0 + 1;
    sl1 = (sl1 + 1 == R) ? 0 : sl1 + 1;
    sl2 = (sl2 + 1 == R) ? 0 : sl2 + 1;
    sdy = (sdy + 1 == NDY) ? 0 : sdy + 1;
  }
  }                                                      // images of this unit
#ifdef UNETDC_WGRAD_STAMPS
  if (lane == 0 && blockIdx.x < 512) {
    unsigned long long* o = g_wgrad_stamps[blockIdx.x][half * 4 + wave];
    o[0] = st_sum[0]; o[1] = st_sum[1]; o[2] = st_kernel0; o[3] = st_sum[3]; o[4] = st_sum[4];
    o[2] = __builtin_amdgcn_s_memtime() - st_kernel0;     // loop time incl. prologue (before the exchange / slab stores)
  }
#endif

  // every DMA has landed (vmcnt(0) on the last step); join of tap 4, (paired form) of the two halves, and the slab stores
  split_finish<HV>(acc, smem, smem_all, half, p, unit, i0, j0, qj, tg, lane);
#endif  // __HIP_DEVICE_COMPILE__
}

template <int PF, bool INORM = false, int HV = 1>
__global__ __launch_bounds__(256 * HV, 2) void wgrad_ring_split_kernel(const WgradFusedParams p) {
  // the tap group is wave-uniform: two specialisations of the whole body, so the 160 accumulator registers of a wave
  // never meet in a phi (a per-step branch made the allocator spill ~590 registers)
  if (__builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 7) & 1)) == 0) ring_split_body<PF, 0, INORM, HV>(p);
  else ring_split_body<PF, 1, INORM, HV>(p);
}

template <int TG, int HV>
__device__ __forceinline__ void fused_split_body(const WgradFusedParams& p) {
#if defined(__HIP_DEVICE_COMPILE__)
  using T = bf16_t;
  constexpr int SEG = SEG_BF16;
  constexpr int XR = SEG + 16;                         // X segment rows (x0-d .. x0+SEG-1+d, d <= 8)
  constexpr int ES = (int)sizeof(T);
  constexpr int RB = 64 * ES;                          // bytes per pixel row (64 channels)
  constexpr int CPR = RB / 16, RPI = 64 / CPR;         // lanes per row, rows per DMA instruction
  constexpr int DYI = SEG / RPI, XI = XR / RPI;        // DMA instructions: dY segment, one X segment
  constexpr int NSLOT = (DYI + 3 * XI + 3) / 4;        // per wave
  constexpr int DYB = SEG * RB, XB = XR * RB;
  constexpr int STAGE = DYB + 3 * XB;
  static_assert(SEG % RPI == 0 && XR % RPI == 0, "segment/instruction mismatch");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
  const int half = HV == 2 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;      // paired form: see split_finish
  unsigned char* const smem = smem_all + half * p.half_lds;

  const int tid = threadIdx.x & 255, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lds_base = lds_addr_of(smem);
  const int qj = wave & 1;
  constexpr int tg = TG;
  // block -> (unit, it, jt); unit -> (image, x segment, y range)
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles = p.itiles * p.jtiles;
  const int unit = L / tiles, trem = L - unit * tiles;
  const int it = trem / p.jtiles, jt = trem - it * p.jtiles;
  const int i0 = it * 64, j0 = jt * 64;
  const int segs = p.W / SEG;
  const int ys = unit % p.ysplit, strip = unit / p.ysplit;
  const int n = strip / segs, x0 = (strip - n * segs) * SEG;
  const int rows_h = HV == 2 ? p.rows_per_unit / 2 : p.rows_per_unit;
  const int ybeg = ys * p.rows_per_unit + half * rows_h;
  const int yend = min(ybeg + rows_h, p.H);

  const unsigned dybytes = (unsigned)((long)p.N * p.H * p.W * p.lddy * ES);
  const unsigned xbytes = (unsigned)((long)p.N * p.H * p.W * p.ldx * ES);
  const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.dy), 0, dybytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, xbytes, 0x00020000);

  // ---- DMA slots of this wave: slot q -> global instruction index gi = wave + 4*q --------------
  //   gi < DYI            : dY segment, instruction gi
  //   gi = DYI + ky*XI + k: X segment ky, instruction k
  const int sub = lane / CPR, pc = lane % CPR;
  unsigned colb[NSLOT];          // byte offset inside the image row (pixel * ld + channel chunk) or FOOB
#pragma unroll
  for (int q = 0; q < NSLOT; ++q) {
    const int gi = wave + 4 * q;
    if (gi < DYI) {
      const int row = gi * RPI + sub;                                  // pixel x0 + row
      const int c = Frag16::src_chunk(row, pc);
      colb[q] = (unsigned)(((x0 + row) * p.lddy + i0) * ES + c * 16);
    } else if (gi < DYI + 3 * XI) {
      const int k = (gi - DYI) % XI;
      const int row = k * RPI + sub;                                   // pixel x0 - d + row
      const int gx = x0 - p.d + row;
      const int c = Frag16::src_chunk(row, pc);
      colb[q] = ((unsigned)gx < (unsigned)p.W) ? (unsigned)((gx * p.ldx + j0) * ES + c * 16) : FOOB;
    } else {
      colb[q] = FOOB;
    }
  }

  SplitAcc acc;
  split_zero(acc);
  const Split16Offs offs = split_offsets(lane, qj, p.d);

  auto issue = [&](int stage, int y) {
#pragma unroll
    for (int q = 0; q < NSLOT; ++q) {
      const int gi = wave + 4 * q;                                     // wave-uniform
      if (gi < DYI) {
        const unsigned rowbase = (unsigned)((long)(n * p.H + y) * p.W * p.lddy * ES);
        lds_dma16(dyr, lds_base + stage * STAGE + gi * 1024, colb[q], rowbase);
      } else if (gi < DYI + 3 * XI) {
        const int ky = (gi - DYI) / XI, k = (gi - DYI) - ky * XI;
        const int yy = y + (ky - 1) * p.d;
        const bool yok = (unsigned)yy < (unsigned)p.H;
        const unsigned rowbase = (unsigned)((long)(n * p.H + (yok ? yy : 0)) * p.W * p.ldx * ES);
        const unsigned v = (yok && colb[q] != FOOB) ? colb[q] : FOOB;
        lds_dma16(xr, lds_base + stage * STAGE + DYB + ky * XB + k * 1024, v, rowbase);
      }
    }
  };

  const int nsteps = yend - ybeg;
  if (nsteps > 0) issue(0, ybeg);
  for (int s = 0; s < nsteps; ++s) {
    wait_vmcnt<0>();                                   // asm DMA + raw barrier: see lds_dma.h
    raw_barrier();
    auto issue_row = [&]() {
      if (s + 1 < nsteps) issue((s + 1) & 1, ybeg + s + 1);
    };
    const unsigned char* sdy = smem + (s & 1) * STAGE;
    const unsigned char* sx = sdy + DYB;
    ring_split_step16<TG>(acc.a, sdy, sx, sx + XB, sx + 2 * XB, offs, issue_row);
  }

  // every DMA has landed (vmcnt(0) on the last step); join of tap 4, (paired form) of the two halves, and the slab stores
  split_finish<HV>(acc, smem, smem_all, half, p, unit, i0, j0, qj, tg, lane);
#endif  // __HIP_DEVICE_COMPILE__
}

// tap-split form of the three-segment kernel (d = 4, 8): same staging, the wave roles of wgrad_ring_split_kernel
template <int HV = 1>
__global__ __launch_bounds__(256 * HV, 2) void wgrad_fused_split_kernel(const WgradFusedParams p) {
  if (__builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 7) & 1)) == 0) fused_split_body<0, HV>(p);
  else fused_split_body<1, HV>(p);
}

// ------------------------------------------------------------------------------------------------
// Host side.  plan_wgrad_fused decides everything about a call -- kernel variant, row split, LDS, grid, slabs -- and
// launch_wgrad_fused only fills the kernel's parameters from that plan.

static int fused_seg(int dtype) { return dtype == UNETDC_BF16 ? SEG_BF16 : SEG_F32; }

// LDS bytes of the ring kernel, or 0 when the configuration does not leave room for two workgroups per CU
static int ring_lds(int d, int dtype, int pf) {
  const int es = dtype == UNETDC_BF16 ? 2 : 4, seg = fused_seg(dtype);
  const int dyb = seg * 64 * es, xb = (seg + 16) * 64 * es;
  const int lds = (pf + 1) * dyb + (2 * d + pf + 1) * xb;
  return lds <= 80 * 1024 ? lds : 0;
}
// prefetch stages of the ring, 0: three-segment staging (fp32: the ring fits at d = 1 with one stage only)
static int ring_pf(int d, int dtype) {
  if (d > 2) return 0;
  if (ring_lds(d, dtype, 2)) return 2;
  if (ring_lds(d, dtype, 1)) return 1;
  return 0;
}

// Rows of the image per unit: about `target` workgroups (`wgs` of them per y range), at least `min_rows` rows each.
struct RowSplit { int rows, ysplit; };
static RowSplit row_split(int H, int wgs, int target, int min_rows) {
  int ys = target / wgs;
  if (ys < 1) ys = 1;
  if (ys > H / min_rows) ys = H / min_rows > 0 ? H / min_rows : 1;
  const int rows = (H + ys - 1) / ys;
  return RowSplit{rows, (H + rows - 1) / rows};
}
// the two row splits of the route: 256-thread workgroups, two per CU; paired 512-thread workgroups, one per CU
static RowSplit single_split(int H, int wgs) { return row_split(H, wgs, 512, 8); }
static RowSplit paired_split(int H, int wgs) { return row_split(H, wgs, 256, 16); }

// The slab bytes of the route for ANY dilation, leading dimensions and normalisation: what the C-ABI workspace query
// promises and what launch_wgrad compares a caller's workspace with.  It is the slab count of the unpaired split, and no
// plan has more slabs than that:
//   * ysplit(y) = ceil(H / ceil(H / y)) does not decrease with y, and the paired split starts from a y that is not larger
//     (256 / wgs <= 512 / wgs, H / 16 <= H / 8, and the clamps keep the order);
//   * walking several images per workgroup (imgs_per_unit) only happens at ysplit == 1 and divides the units further.
// launch_wgrad_fused checks it for the plan it is given.
long wgrad_fused_workspace_bytes(int N, int H, int W, int CI, int CJ, int dtype) {
  const int seg = fused_seg(dtype);
  if (W < seg || W % seg != 0 || H < 1 || CI % 64 != 0 || CJ % 64 != 0) return 0;
  const int strips = N * (W / seg), tiles = (CI / 64) * (CJ / 64);
  return (long)strips * single_split(H, strips * tiles).ysplit * 9 * CI * CJ * 4;
}

WgradFusedPlan plan_wgrad_fused(const WgradParams& w, int dtype) {
  WgradFusedPlan pl{};
  const int N = w.N, H = w.H, W = w.W, CI = w.CI, CJ = w.CJ, d = w.offy[8];
  const bool bf16 = dtype == UNETDC_BF16;
  const int es = bf16 ? 2 : 4, seg = fused_seg(dtype);
  if (w.Hb != H || w.Wb != W || w.ntaps != 9 || w.stride != 1 || d < 1 || d > 8) return pl;
  if (CI % 64 != 0 || CJ % 64 != 0 || CI > 1024 || CJ > 1024 || W % seg != 0) return pl;
  const long P = (long)N * H * W;
  if (P < 32L * 1024 || P * w.lda * es >= (1L << 31) || P * w.ldb * es >= (1L << 31)) return pl;
  pl.pf = ring_pf(d, dtype);
  pl.bnin = w.in_scale != nullptr;
  if (pl.bnin && !(bf16 && pl.pf)) return pl;            // input normalisation: the tap-split ring kernels only
  pl.supported = true;
  pl.workspace = wgrad_fused_workspace_bytes(N, H, W, CI, CJ, dtype);

  const int strips = N * (W / seg), tiles = (CI / 64) * (CJ / 64);
  // 256-thread workgroups, two per CU: the ring where it fits (+ 512 bytes of normalisation constants), else the
  // three-segment staging, double buffered
  RowSplit rs = single_split(H, strips * tiles);
  int target = 512;
  pl.threads = 256;
  pl.lds = pl.pf ? ring_lds(d, dtype, pl.pf) + (pl.bnin ? 512 : 0) : 2 * (seg * 64 * es + 3 * (seg + 16) * 64 * es);
  pl.lds_attr = pl.pf ? (pl.bnin ? 96 : 80) * 1024 : pl.lds;
  // PAIRED FORM (bf16, round 4): 512-thread workgroups whose two halves walk the two halves of a unit's rows and meet in LDS
  // (split_finish): half as many fp32 slabs written and reduced.  One workgroup per CU (the two rings fill the LDS), so
  // every half does exactly the work a 256-thread workgroup does.  Only when the two halves get the same number of rows.
  // (three-segment staging, d = 4 / 8, waits for ALL its DMAs at every step: in lock step the two halves expose that wait
  //  together -- measured 155.4 vs 157.9 us at d = 4 but 175.3 vs 166.3 us at d = 8, profiles/r04_wgrad_pair_ab.txt)
  if (bf16 && (pl.pf || d <= 4)) {
    const RowSplit r2 = paired_split(H, strips * tiles);
    if (r2.rows % 2 == 0 && H % r2.rows == 0 && 2 * pl.lds <= 160 * 1024) {
      pl.paired = true;
      rs = r2;
      target = 256;
      pl.threads = 512;
      pl.half_lds = pl.lds;
      pl.lds = pl.lds_attr = 160 * 1024;                 // two rings, and 144 KB of them for the hand-over at the end
    }
  }
  pl.rows_per_unit = rs.rows;
  pl.ysplit = rs.ysplit;
  pl.units = strips * rs.ysplit;
  // tap-split ring kernels, more workgroups than the target although every one walks a whole image: several images per
  // workgroup
  if (bf16 && pl.pf && rs.ysplit == 1 && (long)pl.units * tiles > target && N > 1) {
    int ipu = (int)(((long)pl.units * tiles + target - 1) / target);
    if (ipu > N) ipu = N;
    pl.imgs_per_unit = ipu;
    pl.units = (W / seg) * ((N + ipu - 1) / ipu);
  }
  pl.nwg = pl.units * tiles;
  return pl;
}

// The kernel of a plan and the name unetdc_last_kernel() reports for it.
struct FusedKernel {
  void (*fn)(const WgradFusedParams);
  const char* name;
};
static FusedKernel fused_kernel(const WgradFusedPlan& pl, int dtype) {
  if (dtype != UNETDC_BF16) {                            // the quadrant kernels
    if (!pl.pf) return {wgrad_fused_kernel, "wgrad_fused_kernel<float>"};
    if (pl.pf == 1) return {wgrad_ring_kernel<1>, "wgrad_ring_kernel<float, 1>"};
    return {nullptr, "wgrad_ring_kernel<float, 2>"};
  }
  if (!pl.pf) {
    if (pl.paired) return {wgrad_fused_split_kernel<2>, "wgrad_fused_split_kernel<16x16x32> paired"};
    return {wgrad_fused_split_kernel<1>, "wgrad_fused_split_kernel<16x16x32>"};
  }
#define RING_SPLIT(PF, INORM, HV, SUFFIX) \
  {wgrad_ring_split_kernel<PF, INORM, HV>, "wgrad_ring_split_kernel<" #PF ", 16x16x32>" SUFFIX}
  static const FusedKernel ring[2][2][2] = {             // [pf - 1][paired][bnin]
      {{RING_SPLIT(1, false, 1, ""), RING_SPLIT(1, true, 1, " bnin")},
       {RING_SPLIT(1, false, 2, " paired"), RING_SPLIT(1, true, 2, " paired bnin")}},
      {{RING_SPLIT(2, false, 1, ""), RING_SPLIT(2, true, 1, " bnin")},
       {RING_SPLIT(2, false, 2, " paired"), RING_SPLIT(2, true, 2, " paired bnin")}}};
#undef RING_SPLIT
  return ring[pl.pf - 1][pl.paired][pl.bnin];
}

// Fills the slabs (dy = w.a, x = w.b); the caller reduces pl.units slabs with wgrad_reduce_kernel.
int launch_wgrad_fused(const WgradParams& w, const WgradFusedPlan& pl, int dtype, hipStream_t stream) {
  const FusedKernel k = fused_kernel(pl, dtype);
  UNETDC_REQUIRE(pl.supported && k.fn, "wgrad_fused: no kernel for this call (%s)", k.name);
  UNETDC_REQUIRE((long)pl.units * 9 * w.CI * w.CJ * 4 <= pl.workspace, "wgrad_fused: %d slabs exceed the workspace bound of %ld bytes",
                 pl.units, pl.workspace);
  WgradFusedParams p{};
  p.dy = w.a; p.x = w.b; p.part = w.part; p.N = w.N; p.H = w.H; p.W = w.W; p.CI = w.CI; p.CJ = w.CJ; p.lddy = w.lda; p.ldx = w.ldb;
  p.d = w.offy[8]; p.in_scale = w.in_scale; p.in_shift = w.in_shift;
  p.ysplit = pl.ysplit; p.rows_per_unit = pl.rows_per_unit; p.itiles = w.CI / 64; p.jtiles = w.CJ / 64;
  p.imgs_per_unit = pl.imgs_per_unit; p.half_lds = pl.half_lds;
  if (const int rc_ = ensure_dynamic_lds(reinterpret_cast<const void*>(k.fn), pl.lds_attr, k.name)) return rc_;
  hipLaunchKernelGGL(k.fn, dim3((unsigned)pl.nwg), dim3(pl.threads), pl.lds, stream, p);
  note_kernel(k.name);
  return check_launch(k.name);
}

}  // namespace unetdc
