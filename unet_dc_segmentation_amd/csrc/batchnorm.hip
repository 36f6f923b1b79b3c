// BatchNorm of the U-Net path: batch statistics -> scale / shift, normalisation (+ReLU, +2x2 max-pool), and the backward
// (with the pool scatter and skip-gradient sum folded in).  All tensors NHWC, every global access is a 16-byte chunk;
// reductions are two-stage with fixed summation order (partials.h).  Each kernel sits next to its launcher.
#include "bn_bwd_terms.h"
#include "partials.h"

namespace unetdc {

// BatchNorm (train): finalize batch statistics  (nn.BatchNorm2d, models/model_2.py:45,52)
//   parts[i][0][c] = partial sum, parts[i][1][c] = partial sum of squares
//   scale = gamma*rstd, shift = beta - mean*scale; running stats use the UNBIASED variance.
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ parts, int nparts, double count,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float momentum,
                                                          float* running_mean, float* running_var, float* scale,
                                                          float* shift, float* mean_out, float* rstd_out, int C) {
  __shared__ double red[4 * 2 * FIN_C], tot[2 * FIN_C];
  const int c4 = blockIdx.x * FIN_C;
  const int nch = min(FIN_C, C - c4);
  double acc[2][FIN_C] = {};
  fin_rows<2>(parts, nparts, C, c4, nch, acc);
  fin_block_sum<2>(acc, red, tot);
  if ((int)threadIdx.x >= nch) return;
  const int c = c4 + threadIdx.x;
  const double s = tot[threadIdx.x], q = tot[FIN_C + threadIdx.x];
  const double mean = s / count;
  double var = q / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[c] * rstd;
  scale[c] = sc;
  shift[c] = beta[c] - (float)mean * sc;
  mean_out[c] = (float)mean;
  rstd_out[c] = rstd;
  if (running_mean) {
    const double unbiased = var * (count / (count > 1.0 ? count - 1.0 : 1.0));
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

int launch_bn_finalize(const float* parts, int nparts, long count, const float* gamma, const float* beta, float eps,
                       float momentum, float* rm, float* rv, float* scale, float* shift, float* mean, float* rstd,
                       int C, hipStream_t stream) {
  UNETDC_REQUIRE(parts && gamma && beta && scale && shift && mean && rstd, "bn_finalize: null pointer");
  UNETDC_REQUIRE(nparts > 0 && count > 0 && C > 0, "bn_finalize: empty problem");
  const float* rp; int rows;
  int rc = reduce_parts(parts, nparts, 2 * C, &rp, &rows, stream, REDUCE_DIRECT_WIDE);
  if (rc != UNETDC_OK) return rc;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + FIN_C - 1) / FIN_C), dim3(256), 0, stream, rp, rows, (double)count, gamma,
                     beta, eps, momentum, rm, rv, scale, shift, mean, rstd, C);
  return check_launch("bn_finalize_kernel");
}

// BatchNorm with FROZEN statistics under autograd (model.eval() with gradients enabled): the training-path kernels run with
// mean / rstd taken from the running buffers instead of the batch; the conv bias is added by the conv epilogue as in training
__global__ void bn_frozen_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                        const float* __restrict__ rm, const float* __restrict__ rv, float eps, float* scale,
                                        float* shift, float* mean, float* rstd, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float r = 1.f / sqrtf(rv[c] + eps);
  const float sc = gamma[c] * r;
  scale[c] = sc;
  shift[c] = beta[c] - rm[c] * sc;
  mean[c] = rm[c];
  rstd[c] = r;
}

int launch_bn_frozen_affine(const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* scale,
                            float* shift, float* mean, float* rstd, int C, hipStream_t stream) {
  UNETDC_REQUIRE(gamma && beta && rm && rv && scale && shift && mean && rstd, "bn_frozen_affine: null pointer");
  hipLaunchKernelGGL(bn_frozen_affine_kernel, dim3((C + 63) / 64), dim3(64), 0, stream, gamma, beta, rm, rv, eps, scale, shift,
                     mean, rstd, C);
  return check_launch("bn_frozen_affine_kernel");
}

// BatchNorm (eval) folded with the conv bias: y = relu(acc*scale + shift)
__global__ void bn_eval_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ rm, const float* __restrict__ rv,
                                      const float* __restrict__ conv_bias, float eps, float* scale, float* shift,
                                      int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s = gamma[c] / sqrtf(rv[c] + eps);
  scale[c] = s;
  shift[c] = beta[c] + ((conv_bias ? conv_bias[c] : 0.f) - rm[c]) * s;
}

int launch_bn_eval_affine(const float* gamma, const float* beta, const float* rm, const float* rv,
                          const float* conv_bias, float eps, float* scale, float* shift, int C, hipStream_t stream) {
  UNETDC_REQUIRE(gamma && beta && rm && rv && scale && shift, "bn_eval_affine: null pointer");
  hipLaunchKernelGGL(bn_eval_affine_kernel, dim3((C + 63) / 64), dim3(64), 0, stream, gamma, beta, rm, rv, conv_bias,
                     eps, scale, shift, C);
  return check_launch("bn_eval_affine_kernel");
}

// a = relu(scale*y + shift)  (or a = y when scale == null), optional 2x2 max-pool of a
//   F.max_pool2d(x, 2): models/model_2.py:59-61,64.   POOL: one thread per (2x2 window, chunk).
template <typename T, bool POOL>
__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const ApplyParams p) {
  constexpr int EPC = Chunk<T>::N;
  const int cpp = p.C / EPC;                                  // chunks per pixel
  const int Hq = POOL ? p.H / 2 : p.H, Wq = POOL ? p.W / 2 : p.W;
  const long total = (long)p.N * Hq * Wq * cpp;
  const T* __restrict__ yg = reinterpret_cast<const T*>(p.y);
  T* __restrict__ ag = reinterpret_cast<T*>(p.a);
  T* __restrict__ pg = reinterpret_cast<T*>(p.pooled);
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int ch = (int)(idx % cpp);
    const long q = idx / cpp;
    const int c0 = ch * EPC;
    float sc[EPC], sh[EPC];
    if (p.scale) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) { sc[e] = p.scale[c0 + e]; sh[e] = p.shift[c0 + e]; }
    }
    if (!POOL) {
      float v[EPC];
      Chunk<T>::unpack(ld16(yg + q * p.ldy + c0), v);
      if (p.scale) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f);
      }
      st16(ag + q * p.lda + c0, Chunk<T>::pack(v));
    } else {
      const int xq = (int)(q % Wq);
      const long t2 = q / Wq;
      const int yq = (int)(t2 % Hq), n = (int)(t2 / Hq);
      float best[EPC];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long pix = ((long)n * p.H + 2 * yq + (k >> 1)) * p.W + 2 * xq + (k & 1);
        float v[EPC];
        Chunk<T>::unpack(ld16(yg + pix * p.ldy + c0), v);
        if (p.scale) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) v[e] = round_through<T>(fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f));
          if (ag) st16(ag + pix * p.lda + c0, Chunk<T>::pack(v));
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) best[e] = (k == 0) ? v[e] : fmaxf(best[e], v[e]);
      }
      st16(pg + q * p.ldp + c0, Chunk<T>::pack(best));
    }
  }
}

int launch_apply(ApplyParams& p, int dtype, hipStream_t stream) {
  const int epc = chunk_elems(dtype);
  UNETDC_REQUIRE(epc, "bn_relu_apply: bad dtype %d", dtype);
  UNETDC_REQUIRE(p.y, "bn_relu_apply: null input");
  UNETDC_REQUIRE(p.C % epc == 0 && p.ldy % epc == 0, "bn_relu_apply: C/ld not chunk aligned");
  UNETDC_REQUIRE((p.scale == nullptr) == (p.shift == nullptr), "bn_relu_apply: scale/shift mismatch");
  const bool pool = p.pooled != nullptr;
  if (pool) UNETDC_REQUIRE(p.H % 2 == 0 && p.W % 2 == 0 && p.ldp % epc == 0, "bn_relu_apply: pooling needs even H, W");
  if (!pool) UNETDC_REQUIRE(p.a != nullptr, "bn_relu_apply: nothing to write");
  if (p.a) UNETDC_REQUIRE(p.lda % epc == 0, "bn_relu_apply: lda not chunk aligned");
  const long items = (long)p.N * (pool ? p.H / 2 : p.H) * (pool ? p.W / 2 : p.W) * (p.C / epc);
  const int nb = grid_for(items, 256);
  dispatch(dtype, [&](auto t, auto pooling) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((bn_relu_apply_kernel<T, decltype(pooling)::value>), dim3(nb), dim3(256), 0, stream, p);
  }, pool);
  return check_launch("bn_relu_apply_kernel");
}

// BatchNorm+ReLU backward.  Incoming gradient dA of the activated output a = relu(scale*y+shift):
//     dA = dskip (+ scatter of dpool to the window arg-max when POOL)
//   dyhat = dA * [a > 0];  xhat = (y - mean)*rstd
//   reduce:   S1 = sum dyhat, S2 = sum dyhat*xhat, S3 = sum xhat      (per channel)
//   apply:    dy = k1*dyhat - k2 - k3*xhat,   k1 = gamma*rstd, k2 = k1*S1/M, k3 = k1*S2/M
//   dgamma = S2, dbeta = S1, dbias(conv) = sum dy = -k3*S3  (zero up to rounding, as in the reference)
// The pool arg-max is recomputed from y exactly as the forward pass saw it (values rounded through
// the storage type, first maximum in row-major window order: ATen's tie rule).
// HEAD (non-pooled apply pass only): the incoming gradient is recomputed from the head's dprobs / probs / weight row
// (BnBwdParams::head_w) -- a template parameter, because the extra registers and the branch cost the plain form 40 % as a
// run-time switch
template <typename T, bool POOL, bool APPLY, bool HEAD = false>
__global__ __launch_bounds__(256) void bn_bwd_kernel(const BnBwdParams p) {
  static_assert(!HEAD || (!POOL && APPLY), "head form: non-pooled apply pass");
  constexpr int EPC = Chunk<T>::N;
  __shared__ float red[256 * 3 * EPC];
  const int cpp = p.C / EPC;
  const int tid = threadIdx.x;
  // thread -> fixed channel chunk; pixel lanes stride over the (window) list
  const int seg = (cpp < 256) ? cpp : 256;                 // chunk lanes per block row
  const int plane = 256 / seg;                             // pixel lanes
  const int chl = tid % seg, pl = tid / seg;
  const int ch = blockIdx.y * seg + chl;
  const bool active = (pl < plane) && (ch < cpp);
  const int c0 = ch * EPC;
  const int Hq = POOL ? p.H / 2 : p.H, Wq = POOL ? p.W / 2 : p.W;
  const long Q = (long)p.N * Hq * Wq;
  const T* __restrict__ yg = reinterpret_cast<const T*>(p.y);
  const T* __restrict__ sg = reinterpret_cast<const T*>(p.dskip);
  const T* __restrict__ dpg = reinterpret_cast<const T*>(p.dpool);
  T* __restrict__ dyg = reinterpret_cast<T*>(p.dy);

  float sc[EPC], sh[EPC], mu[EPC], rs[EPC], k1[EPC], k2[EPC], k3[EPC], hw[EPC];
  float s1[EPC], s2[EPC], s3[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    s1[e] = s2[e] = s3[e] = 0.f;
    hw[e] = 0.f;
    if (active) {
      sc[e] = p.scale[c0 + e]; sh[e] = p.shift[c0 + e]; mu[e] = p.mean[c0 + e]; rs[e] = p.rstd[c0 + e];
      if (APPLY) { k1[e] = p.k1[c0 + e]; k2[e] = p.k2[c0 + e]; k3[e] = p.k3[c0 + e]; }
      if (HEAD) hw[e] = p.head_w[c0 + e];
    }
  }
  if (active) {
    for (long q = (long)blockIdx.x * plane + pl; q < Q; q += (long)gridDim.x * plane) {
      if (!POOL) {
        float yv[EPC], g[EPC];
        Chunk<T>::unpack(ld16(yg + q * p.ldy + c0), yv);
        if (HEAD) {                                        // gradient of the head's input, recomputed (see BnBwdParams)
          const float pr = p.head_probs[q];
          const float dz = p.head_dprobs[q] * pr * (1.f - pr);
#pragma unroll
          for (int e = 0; e < EPC; ++e) g[e] = round_through<T>(dz * hw[e]);
        } else {
          Chunk<T>::unpack(ld16(sg + q * p.lds + c0), g);
        }
        float out[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const float gh = bn_dyhat(bn_nrm(yv[e], sc[e], sh[e]), g[e]);
          const float xh = bn_xhat(yv[e], mu[e], rs[e]);
          if (APPLY) out[e] = bn_bwd_apply(k1[e], k2[e], k3[e], gh, xh);
          else bn_bwd_sums(gh, xh, s1[e], s2[e], s3[e]);
        }
        if (APPLY) st16(dyg + q * p.lddy + c0, Chunk<T>::pack(out));
      } else {
        // The nine 16-byte chunks of a window (4 x y, 4 x dskip, dpool) stay RAW and every channel is taken out of them when
        // its turn comes: holding them unpacked cost 160 / 192 registers (3 / 2 waves per SIMD on a pass that lives on
        // memory-level parallelism).  Arithmetic and summation order per channel are unchanged.
        const int xq = (int)(q % Wq);
        const long t2 = q / Wq;
        const int yq = (int)(t2 % Hq), n = (int)(t2 / Hq);
        long pix[4];
        u32x4 yr[4], sr[4], dpr, outr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pix[k] = ((long)n * p.H + 2 * yq + (k >> 1)) * p.W + 2 * xq + (k & 1);
          yr[k] = ld16(yg + pix[k] * p.ldy + c0);
        }
        dpr = ld16(dpg + q * p.ldp + c0);
        if (sg) {
#pragma unroll
          for (int k = 0; k < 4; ++k) sr[k] = ld16(sg + pix[k] * p.lds + c0);
        }
        float prev[4] = {0.f, 0.f, 0.f, 0.f};               // APPLY, bf16: the even element of a pair waits for the odd one
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          float yk[4], nrm[4];
          float best = 0.f;
          int arg = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            yk[k] = chunk_elem<T>(yr[k], e);
            nrm[k] = bn_nrm(yk[k], sc[e], sh[e]);
            const float a = round_through<T>(fmaxf(nrm[k], 0.f));
            if (k == 0 || a > best) { best = a; arg = k; }
          }
          const float dpe = chunk_elem<T>(dpr, e);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float gin = (sg ? chunk_elem<T>(sr[k], e) : 0.f) + (arg == k ? dpe : 0.f);
            const float gh = bn_dyhat(nrm[k], gin);
            const float xh = bn_xhat(yk[k], mu[e], rs[e]);
            if (APPLY) chunk_set<T>(outr[k], e, bn_bwd_apply(k1[e], k2[e], k3[e], gh, xh), prev[k]);
            else bn_bwd_sums(gh, xh, s1[e], s2[e], s3[e]);
          }
        }
        if (APPLY) {
#pragma unroll
          for (int k = 0; k < 4; ++k) st16(dyg + pix[k] * p.lddy + c0, outr[k]);
        }
      }
    }
  }
  if (!APPLY) {
    // block reduction over pixel lanes (fixed order)
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      red[(tid * 3 + 0) * EPC + e] = s1[e];
      red[(tid * 3 + 1) * EPC + e] = s2[e];
      red[(tid * 3 + 2) * EPC + e] = s3[e];
    }
    __syncthreads();
    // one thread per (chunk lane, which, element)
    for (int i = tid; i < seg * 3 * EPC; i += 256) {
      const int cl = i / (3 * EPC), rem = i - cl * 3 * EPC, which = rem / EPC, e = rem - which * EPC;
      const int chn = blockIdx.y * seg + cl;
      if (chn >= cpp) continue;
      float s = 0.f;
      for (int q2 = 0; q2 < plane; ++q2) s += red[((q2 * seg + cl) * 3 + which) * EPC + e];
      p.parts[((long)blockIdx.x * 3 + which) * p.C + chn * EPC + e] = s;
    }
  }
}

BnBwdPlan plan_bn_bwd(int N, int H, int W, int C, int pooled, int dtype) {
  BnBwdPlan pl{};
  pl.epc = chunk_elems(dtype);
  if (!pl.epc || C <= 0 || C % pl.epc) return pl;
  pl.cpp = C / pl.epc; pl.seg = pl.cpp < 256 ? pl.cpp : 256;
  if (256 % pl.seg) return pl;
  const long Q = (long)N * (pooled ? H / 2 : H) * (pooled ? W / 2 : W);
  const long per = (long)(256 / pl.seg) * 8;                   // >= 8 items per pixel lane
  const long nb = (Q + per - 1) / per;
  pl.nb = (int)(nb > 512 ? 512 : nb < 1 ? 1 : nb);
  pl.ny = (pl.cpp + pl.seg - 1) / pl.seg;
  pl.apply_nb = grid_for(Q * pl.cpp, 256) > 4096 ? 4096 : grid_for(Q * pl.cpp, 256);
  pl.workspace = (partial_floats(pl.nb, 3L * C) + 3L * C) * 4;
  pl.ok = true;
  return pl;
}

// head only with !pool && apply (launch_bn_bwd checks): the other combinations of HEAD stay uninstantiated
static void launch_bn_bwd_k(const BnBwdParams& p, int dtype, bool pool, bool apply, bool head, dim3 grid, hipStream_t stream) {
  dispatch(dtype, [&](auto t, auto P, auto A, auto Hd) {
    using T = typename decltype(t)::type;
    constexpr bool POOL = decltype(P)::value, APPLY = decltype(A)::value, HEAD = decltype(Hd)::value;
    if constexpr (!HEAD || (!POOL && APPLY))
      hipLaunchKernelGGL((bn_bwd_kernel<T, POOL, APPLY, HEAD>), grid, dim3(256), 0, stream, p);
  }, pool, apply, head);
}

// Reduction pass only: fills `parts` ([nparts][3][C]) -- used when the producer kernel could not fuse it.
int launch_bn_bwd_reduce_only(BnBwdParams& p, float* parts, long parts_floats, int* nparts, int dtype, hipStream_t stream) {
  const BnBwdPlan pl = plan_bn_bwd(p.N, p.H, p.W, p.C, 0, dtype);
  UNETDC_REQUIRE(p.y && p.dskip && parts && nparts, "bn_bwd_reduce: null pointer");
  UNETDC_REQUIRE(pl.ok, "bn_bwd_reduce: C=%d unsupported", p.C);
  // the caller sized `parts` for the fused-epilogue producer (one row per 256 pixels + the spare rows); this
  // stand-alone pass (grid-stride over pixels) takes as many workgroups as that buffer has rows for
  const long cap = partial_row_cap(parts_floats, 3L * p.C);
  const int nb = pl.nb > cap ? (int)cap : pl.nb;
  UNETDC_REQUIRE(nb >= 1, "bn_bwd_reduce: partial buffer too small");
  p.parts = parts;
  p.dpool = nullptr;
  launch_bn_bwd_k(p, dtype, false, false, false, dim3(nb, pl.ny), stream);
  *nparts = nb;
  return check_launch("bn_bwd_kernel(reduce)");
}

// dgamma / dbeta / dbias and the coefficients k[3][C] of the apply arithmetic from [nparts][3][C] partial rows
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ parts, int nparts, double count,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ rstd, float* dgamma,
                                                              float* dbeta, float* dbias, float* k1, float* k2,
                                                              float* k3, int C, int frozen) {
  __shared__ double red[4 * 3 * FIN_C], tot[3 * FIN_C];
  const int c4 = blockIdx.x * FIN_C;
  const int nch = min(FIN_C, C - c4);
  double acc[3][FIN_C] = {};
  fin_rows<3>(parts, nparts, C, c4, nch, acc);
  fin_block_sum<3>(acc, red, tot);
  if ((int)threadIdx.x >= nch) return;
  const int c = c4 + threadIdx.x;
  const double s1 = tot[threadIdx.x], s2 = tot[FIN_C + threadIdx.x], s3 = tot[2 * FIN_C + threadIdx.x];
  const double a = (double)gamma[c] * (double)rstd[c];
  dgamma[c] = (float)s2;
  dbeta[c] = (float)s1;
  k1[c] = (float)a;
  if (frozen) {
    // statistics that do not depend on the batch (eval-mode BatchNorm under autograd: running mean / variance): the
    // normalisation is a fixed per-channel affine map, dy = gamma * rstd * dyhat, and the conv bias sees sum(dy)
    k2[c] = 0.f;
    k3[c] = 0.f;
    if (dbias) dbias[c] = (float)(a * s1);
    return;
  }
  k2[c] = (float)(a * s1 / count);
  k3[c] = (float)(a * s2 / count);
  if (dbias) dbias[c] = (float)(-(a * s2 / count) * s3);
}

static int bn_bwd_finalize(const float* parts, int nparts, double count, const float* gamma, const float* rstd, float* dgamma,
                           float* dbeta, float* dbias, float* k, int C, bool frozen, hipStream_t stream) {
  const float* rp; int rows;
  const int rc = reduce_parts(parts, nparts, 3 * C, &rp, &rows, stream, REDUCE_DIRECT_WIDE);
  if (rc != UNETDC_OK) return rc;
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + FIN_C - 1) / FIN_C), dim3(256), 0, stream, rp, rows, count, gamma, rstd,
                     dgamma, dbeta, dbias, k, k + C, k + 2 * C, C, frozen ? 1 : 0);
  return check_launch("bn_bwd_finalize_kernel");
}

int launch_bn_bwd(BnBwdParams& p, const float* gamma, float* dgamma, float* dbeta, float* dbias, void* workspace,
                  long workspace_bytes, const float* pre_parts, int pre_nparts, int dtype, hipStream_t stream, bool frozen) {
  const bool pool = p.dpool != nullptr;
  const BnBwdPlan pl = plan_bn_bwd(p.N, p.H, p.W, p.C, pool, dtype);
  const int epc = pl.epc;
  UNETDC_REQUIRE(epc, "bn_bwd: bad dtype %d", dtype);
  UNETDC_REQUIRE(p.y && p.dy && (p.dskip || p.dpool || p.head_w), "bn_bwd: null tensor");
  if (p.head_w)
    UNETDC_REQUIRE(!p.dskip && !p.dpool && p.head_dprobs && p.head_probs && pre_parts,
                   "bn_bwd (head): needs dprobs, probs and the sums from unetdc_head_bwd_bnstats, and no stored gradient");
  UNETDC_REQUIRE(p.scale && p.shift && p.mean && p.rstd && gamma && dgamma && dbeta && workspace, "bn_bwd: null pointer");
  UNETDC_REQUIRE(p.C % epc == 0 && p.ldy % epc == 0 && p.lddy % epc == 0, "bn_bwd: C/ld not chunk aligned");
  if (pool) UNETDC_REQUIRE(p.H % 2 == 0 && p.W % 2 == 0 && p.ldp % epc == 0, "bn_bwd: pooling needs even H, W");
  if (!pool) UNETDC_REQUIRE(p.dskip != nullptr || p.head_w != nullptr, "bn_bwd: gradient missing");
  if (p.dskip) UNETDC_REQUIRE(p.lds % epc == 0, "bn_bwd: lds not chunk aligned");
  if (pre_parts) UNETDC_REQUIRE(!pool && pre_nparts > 0, "bn_bwd: precomputed partial sums need the non-pooled form");
  UNETDC_REQUIRE(pl.ok, "bn_bwd: C=%d unsupported (C/%d must divide 256 or be a multiple of 256)", p.C, epc);
  if (pl.workspace > workspace_bytes) {
    set_error("bn_bwd: workspace too small (%ld < %ld bytes)", workspace_bytes, pl.workspace);
    return UNETDC_EWORKSPACE;
  }
  float* k = reinterpret_cast<float*>(workspace);          // k1, k2, k3, then the partial rows
  p.parts = k + 3 * p.C;
  p.k1 = k; p.k2 = k + p.C; p.k3 = k + 2 * p.C;
  if (!pre_parts) {       // else: the reduction was fused into the epilogue of the kernel that produced the gradient
    launch_bn_bwd_k(p, dtype, pool, false, false, dim3(pl.nb, pl.ny), stream);
    const int rc = check_launch("bn_bwd_kernel(reduce)");
    if (rc != UNETDC_OK) return rc;
  }
  const int rc = bn_bwd_finalize(pre_parts ? pre_parts : p.parts, pre_parts ? pre_nparts : pl.nb, (double)p.N * p.H * p.W, gamma,
                                 p.rstd, dgamma, dbeta, dbias, k, p.C, frozen, stream);
  if (rc != UNETDC_OK) return rc;
  launch_bn_bwd_k(p, dtype, pool, true, p.head_w != nullptr, dim3(pl.apply_nb, pl.ny), stream);
  return check_launch(p.head_w ? "bn_bwd_kernel(apply, head)" : "bn_bwd_kernel(apply)");
}

// Finalisation alone: dgamma / dbeta / dbias and the three per-channel coefficients of the apply arithmetic
// (dy = k1 * dyhat - k2 - k3 * xhat) into coeffs[3][C], from sums a producer kernel left as partial rows -- for a consumer
// that applies them itself (first-layer weight gradient, first_conv.hip)
int launch_bn_bwd_coeffs(const float* pre_parts, int pre_nparts, long count, const float* gamma, const float* rstd, float* dgamma,
                         float* dbeta, float* dbias, float* coeffs, int C, hipStream_t stream) {
  UNETDC_REQUIRE(pre_parts && pre_nparts > 0 && gamma && rstd && dgamma && dbeta && coeffs && C > 0 && count > 0,
                 "bn_bwd_coeffs: null pointer / empty problem");
  return bn_bwd_finalize(pre_parts, pre_nparts, (double)count, gamma, rstd, dgamma, dbeta, dbias, coeffs, C, false, stream);
}

}  // namespace unetdc
