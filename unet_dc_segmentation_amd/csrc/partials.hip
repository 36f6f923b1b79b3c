// Partial-row reductions: the first-stage reducer (partials.h), column sums of statistics rows, per-channel sums of a tensor.
#include "partials.h"

namespace unetdc {

// column sums of a [nrows][L] fp32 matrix into R row groups: out[r][l] = sum_{i in group r} in[i][l]
__global__ __launch_bounds__(256) void colsum_stage_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           int nrows, int L, int rows_per_group) {
  __shared__ float red[8][33];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cl, grp = blockIdx.y;
  const int rbeg = grp * rows_per_group;
  const int rend = min(rbeg + rows_per_group, nrows);
  float s = 0.f;
  if (col < L)
    for (int i = rbeg + rl; i < rend; i += 8) s += in[(long)i * L + col];
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && col < L) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) t += red[q][cl];
    out[(long)grp * L + col] = t;
  }
}

int reduce_parts(const float* parts, int nparts, int L, const float** red_ptr, int* red_rows, hipStream_t stream, int direct) {
  if (nparts <= direct) {
    *red_ptr = parts;
    *red_rows = nparts;
    return UNETDC_OK;
  }
  float* out = const_cast<float*>(parts) + (long)nparts * L;
  const int rpg = (nparts + SPARE_ROWS - 1) / SPARE_ROWS;
  const int groups = (nparts + rpg - 1) / rpg;
  hipLaunchKernelGGL(colsum_stage_kernel, dim3((L + 31) / 32, groups), dim3(256), 0, stream, parts, out, nparts, L, rpg);
  *red_ptr = out;
  *red_rows = groups;
  return check_launch("colsum_stage_kernel");
}

// Column sums out of MODE_STATS partial rows [nparts][2][L/2 ... ] (row 0 of each pair = sums of the stored values):
// out[c] = sum_rows parts[row][0][c0 + c].  Used for the ConvTranspose2d bias gradient, whose input (the first
// half of the decoder's concat gradient) is written by the dgrad kernel that produced `parts`.
__global__ __launch_bounds__(256) void stats_colsum_finalize_kernel(const float* __restrict__ parts, int nparts, int L, int c0,
                                                                    float* out, int C) {
  // 32 lanes per channel (rows l, l+32, ... each, fixed shuffle tree): a serial walk over the rows cost 15 us per launch
  const int c = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
  double s = 0.0;
  if (c < C)
    for (int i = l; i < nparts; i += 32) s += (double)parts[(long)i * L + c0 + c];
  s = lane32_sum(s);
  if (c < C && l == 0) out[c] = (float)s;
}

int launch_stats_colsum(const float* parts, int nparts, int ctotal, int c0, int c, float* out, hipStream_t stream) {
  UNETDC_REQUIRE(c0 + c <= ctotal, "stats_colsum: bad column range");
  UNETDC_REQUIRE(parts && out && nparts > 0 && c0 >= 0 && c > 0, "stats_colsum: bad arguments");
  const int L = 2 * ctotal;                     // floats per statistics row
  const float* rp; int rows;
  int rc = reduce_parts(parts, nparts, L, &rp, &rows, stream, REDUCE_DIRECT_WIDE);
  if (rc != UNETDC_OK) return rc;
  hipLaunchKernelGGL(stats_colsum_finalize_kernel, dim3((c + 7) / 8), dim3(256), 0, stream, rp, rows, L, c0, out, c);
  return check_launch("stats_colsum_finalize_kernel");
}

// per-channel sum over pixels of an NHWC tensor (ConvTranspose2d bias gradient)
// parts layout: [gridDim.x][C]
template <typename T>
__global__ __launch_bounds__(256) void channel_sum_kernel(const void* __restrict__ x, int ldx, float* __restrict__ parts,
                                                          long P, int C) {
  constexpr int EPC = Chunk<T>::N;
  __shared__ float red[256 * EPC];
  const int cpp = C / EPC;
  const int tid = threadIdx.x;
  const int seg = (cpp < 256) ? cpp : 256, plane = 256 / seg;
  const int chl = tid % seg, pl = tid / seg;
  const int ch = blockIdx.y * seg + chl;
  const T* __restrict__ xg = reinterpret_cast<const T*>(x);
  float s[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) s[e] = 0.f;
  if (ch < cpp)
    for (long q = (long)blockIdx.x * plane + pl; q < P; q += (long)gridDim.x * plane) {
      float v[EPC];
      Chunk<T>::unpack(ld16(xg + q * ldx + ch * EPC), v);
#pragma unroll
      for (int e = 0; e < EPC; ++e) s[e] += v[e];
    }
#pragma unroll
  for (int e = 0; e < EPC; ++e) red[tid * EPC + e] = s[e];
  __syncthreads();
  for (int i = tid; i < seg * EPC; i += 256) {
    const int cl = i / EPC, e = i - cl * EPC;
    const int chn = blockIdx.y * seg + cl;
    if (chn >= cpp) continue;
    float t = 0.f;
    for (int q2 = 0; q2 < plane; ++q2) t += red[(q2 * seg + cl) * EPC + e];
    parts[(long)blockIdx.x * C + chn * EPC + e] = t;
  }
}

__global__ void channel_sum_finalize_kernel(const float* __restrict__ parts, int nparts, float* out, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int i = 0; i < nparts; ++i) s += (double)parts[(long)i * C + c];
  out[c] = (float)s;
}

ChannelSumPlan plan_channel_sum(long P, int C, int dtype) {
  ChannelSumPlan pl{};
  pl.epc = chunk_elems(dtype);
  if (!pl.epc || C <= 0 || C % pl.epc) return pl;
  const int cpp = C / pl.epc, seg = cpp < 256 ? cpp : 256;
  if (256 % seg) return pl;
  pl.nb = (int)std::min(std::max((P + 63) / 64, 1L), 512L);
  pl.ny = (cpp + seg - 1) / seg;
  pl.workspace = partial_floats(pl.nb, C) * 4;
  pl.ok = true;
  return pl;
}

int launch_channel_sum(const void* x, int ldx, float* out, void* workspace, long workspace_bytes, long P, int C,
                       int dtype, hipStream_t stream) {
  const ChannelSumPlan pl = plan_channel_sum(P, C, dtype);
  UNETDC_REQUIRE(pl.epc, "channel_sum: bad dtype %d", dtype);
  UNETDC_REQUIRE(x && out && workspace && P > 0, "channel_sum: null pointer / empty");
  UNETDC_REQUIRE(C % pl.epc == 0 && ldx % pl.epc == 0, "channel_sum: C/ld not chunk aligned");
  UNETDC_REQUIRE(pl.ok, "channel_sum: C=%d unsupported", C);
  if (int rc = require_workspace("channel_sum", workspace_bytes, pl.workspace)) return rc;
  float* parts = reinterpret_cast<float*>(workspace);
  dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(channel_sum_kernel<T>, dim3(pl.nb, pl.ny), dim3(256), 0, stream, x, ldx, parts, P, C);
  });
  int rc = check_launch("channel_sum_kernel");
  if (rc != UNETDC_OK) return rc;
  const float* rp; int rows;
  rc = reduce_parts(parts, pl.nb, C, &rp, &rows, stream, REDUCE_DIRECT);
  if (rc != UNETDC_OK) return rc;
  hipLaunchKernelGGL(channel_sum_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, stream, rp, rows, out, C);
  return check_launch("channel_sum_finalize_kernel");
}

}  // namespace unetdc
