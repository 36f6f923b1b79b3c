// The 1x1 sigmoid head of the U-Net path, forward and backward (optionally with the BatchNorm-backward sums of the stage in
// front of it fused in).  Tensors NHWC, 16-byte chunks; two-stage reductions with fixed summation order (partials.h).
#include "bn_bwd_terms.h"
#include "partials.h"

namespace unetdc {

// Head: 1x1 conv (C -> OC) + sigmoid (models/model_2.py:32,79-80), probabilities out in NCHW fp32.
// C/EPC lanes cooperate on one pixel (C = 64: 8 lanes bf16 / 16 lanes fp32), shuffle-reduced.
// NORM: `a` is the raw conv output of the producing stage and the BatchNorm + ReLU of that stage is applied on load,
// a = relu(scale * y + shift) rounded through the storage type (exactly the values a stand-alone normalisation pass
// would have stored): the activation tensor is never written or read.
template <typename T, bool NORM, int CPP>
__global__ __launch_bounds__(256) void head_fwd_kernel(const HeadParams p) {
  constexpr int EPC = Chunk<T>::N;
  constexpr int UNR = 4;                              // pixels per lane group and trip: four 16-byte loads in flight
  const int cpp = CPP ? CPP : p.C / EPC;              // lanes per pixel (power of two, <= 64); CPP > 0: known at compile time
  const int ppb = 256 / cpp;
  const int tid = threadIdx.x, cl = tid % cpp, pl = tid / cpp;
  const long HW = (long)p.H * p.W, P = (long)p.N * HW;
  const T* __restrict__ ag = reinterpret_cast<const T*>(p.a);
  float nsc[EPC], nsh[EPC];
  if (NORM) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) { nsc[e] = p.bn_scale[cl * EPC + e]; nsh[e] = p.bn_shift[cl * EPC + e]; }
  }
  for (long pb = (long)blockIdx.x * ppb * UNR; pb < P; pb += (long)gridDim.x * ppb * UNR) {
    float v[UNR][EPC];
    long pix[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      pix[u] = pb + u * ppb + pl;
      if (pix[u] < P) Chunk<T>::unpack(ld16(ag + pix[u] * p.lda + cl * EPC), v[u]);
    }
    if (NORM) {
#pragma unroll
      for (int u = 0; u < UNR; ++u)
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[u][e] = round_through<T>(fmaxf(fmaf(v[u][e], nsc[e], nsh[e]), 0.f));
    }
    for (int oc = 0; oc < p.OC; ++oc) {
      float wv[EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) wv[e] = p.w[oc * p.C + cl * EPC + e];
      const float bias = p.b[oc];
      // the four dot products of a trip are reduced TOGETHER, step by step: four independent shuffle chains instead of four
      // serial ones (a cross-lane step is an LDS-crossbar round trip; with a runtime lane count the loop was not unrolled
      // and the kernel ran at 2.9 TB/s on shuffle latency)
      float sv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        sv[u] = 0.f;
        if (pix[u] < P) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) sv[u] = fmaf(v[u][e], wv[e], sv[u]);
        }
      }
      if (CPP) {
#pragma unroll
        for (int o = 1; o < (CPP ? CPP : 1); o <<= 1)
#pragma unroll
          for (int u = 0; u < UNR; ++u) sv[u] += __shfl_xor(sv[u], o, 64);
      } else {
        for (int o = 1; o < cpp; o <<= 1)
#pragma unroll
          for (int u = 0; u < UNR; ++u) sv[u] += __shfl_xor(sv[u], o, 64);
      }
      // every lane of the group holds the four sums: lane u finishes pixel u (sigmoid + store)
      if (cpp >= UNR) {
        float z = sv[0];
#pragma unroll
        for (int u = 1; u < UNR; ++u) z = (cl == u) ? sv[u] : z;
        if (cl < UNR) {
          const long px = pb + cl * ppb + pl;
          if (px < P) {
            const long n = px / HW, rem = px - n * HW;
            p.probs[(n * p.OC + oc) * HW + rem] = 1.f / (1.f + expf(-(z + bias)));
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < UNR; ++u)
          if (pix[u] < P && cl == 0) {
            const long n = pix[u] / HW, rem = pix[u] - n * HW;
            p.probs[(n * p.OC + oc) * HW + rem] = 1.f / (1.f + expf(-(sv[u] + bias)));
          }
      }
    }
  }
}

// dz = dp * p * (1-p);  dA[pix][c] = sum_oc dz[oc]*w[oc][c];  partial sums of dz*a (dW) and dz (db)
// parts layout: [gridDim.x][OC][C + 1]   (last column = bias gradient)
// LEAN (the training path of the networks: one output channel, activation recomputed from y, input gradient not stored): the
// saved output stays a RAW chunk and each channel is taken out of it in turn -- 158 -> fewer registers, i.e. every workgroup of
// the 1024 resident at once instead of three quarters of them.  Same arithmetic, same order.
template <typename T, bool BN, bool LEAN = false>
__global__ __launch_bounds__(256) void head_bwd_kernel(const HeadParams p) {
  static_assert(!LEAN || BN, "lean form: fused BatchNorm-backward sums");
  constexpr int EPC = Chunk<T>::N;
  __shared__ float red[256 * (EPC + 1)];
  __shared__ float red3[BN ? 256 * 3 * EPC : 1];
  const int cpp = p.C / EPC, ppb = 256 / cpp;
  const int tid = threadIdx.x, cl = tid % cpp, pl = tid / cpp;
  const long HW = (long)p.H * p.W, P = (long)p.N * HW;
  const T* __restrict__ ag = reinterpret_cast<const T*>(p.a);
  T* __restrict__ dag = reinterpret_cast<T*>(p.da);
  // BN: the gradient written here is the activation gradient of the stage that produced `a`; its BatchNorm-backward
  // sums (S1 = sum dyhat, S2 = sum dyhat*xhat, S3 = sum xhat: see bn_bwd_kernel) are taken from the value as STORED
  // (rounded through the storage type), so the stand-alone reduction pass over da and y is not needed.
  const T* __restrict__ yg = reinterpret_cast<const T*>(p.bn_y);
  float sc[EPC], sh[EPC], mu[EPC], rs[EPC], s1[EPC], s2[EPC], s3[EPC];
  if (BN) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int c = cl * EPC + e;
      sc[e] = p.bn_scale[c]; sh[e] = p.bn_shift[c]; mu[e] = p.bn_mean[c]; rs[e] = p.bn_rstd[c];
      s1[e] = s2[e] = s3[e] = 0.f;
    }
  }
  for (int oc = 0; oc < p.OC; ++oc) {
    const bool last = oc == p.OC - 1;
    float wv[EPC], gw[EPC], gb = 0.f;
#pragma unroll
    for (int e = 0; e < EPC; ++e) { wv[e] = p.w[oc * p.C + cl * EPC + e]; gw[e] = 0.f; }
    // two pixels per lane group and trip: every load of both is issued before the arithmetic of the first (one 16-byte load
    // in flight per lane at 3 waves per SIMD left the kernel latency bound at 3.4 TB/s)
    constexpr int U = 2;
    if (LEAN) {
      for (long pb = (long)blockIdx.x * ppb * U; pb < P; pb += (long)gridDim.x * ppb * U) {
        u32x4 yraw[U];
        float pr[U], dpv[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long px0 = pb + u * ppb + pl;
          ok[u] = px0 < P;
          const long px = ok[u] ? px0 : 0;
          pr[u] = p.probs[px];                             // OC == 1: [N, 1, H, W] is the pixel index itself
          dpv[u] = p.dprobs[px];
          yraw[u] = ld16(yg + px * p.bn_ldy + cl * EPC);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (!ok[u]) continue;
          float dz = dpv[u] * pr[u] * (1.f - pr[u]);
          asm volatile("" : "+v"(dz));                     // a rounded product, as in the stored form: no contraction into `gb += dz`
#pragma unroll
          for (int e = 0; e < EPC; ++e) {
            const float yv = chunk_elem<T>(yraw[u], e);
            const float nrm = bn_nrm(yv, sc[e], sh[e]);
            const float av = round_through<T>(fmaxf(nrm, 0.f));
            gw[e] = fmaf(dz, av, gw[e]);
            const float g = round_through<T>(0.f + dz * wv[e]);
            const float gh = bn_dyhat(nrm, g);
            const float xh = bn_xhat(yv, mu[e], rs[e]);
            bn_bwd_sums(gh, xh, s1[e], s2[e], s3[e]);
          }
          if (cl == 0) gb += dz;
        }
      }
    } else
    for (long pb = (long)blockIdx.x * ppb * U; pb < P; pb += (long)gridDim.x * ppb * U) {
      long pix[U];
      bool ok[U];
      u32x4 yraw[U], araw[U];
      float pr[U], dpv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pix[u] = pb + u * ppb + pl;
        ok[u] = pix[u] < P;
        const long px = ok[u] ? pix[u] : 0;
        const long n = px / HW, rem = px - n * HW;
        const long o = (n * p.OC + oc) * HW + rem;
        pr[u] = p.probs[o];
        dpv[u] = p.dprobs[o];
        if (BN && (last || !ag)) yraw[u] = ld16(yg + px * p.bn_ldy + cl * EPC);
        if (!BN || ag) araw[u] = ld16(ag + px * p.lda + cl * EPC);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
        float dz = dpv[u] * pr[u] * (1.f - pr[u]);
        asm volatile("" : "+v"(dz));                       // a rounded product in every form: no contraction into `gb += dz`
        float av[EPC], d[EPC], yv[EPC];
        if (BN && (last || !ag)) Chunk<T>::unpack(yraw[u], yv);
        if (!BN || ag) Chunk<T>::unpack(araw[u], av);
        else {                                           // the activation as the forward pass saw it, from the saved conv output
#pragma unroll
          for (int e = 0; e < EPC; ++e) av[e] = round_through<T>(fmaxf(fmaf(yv[e], sc[e], sh[e]), 0.f));
        }
#pragma unroll
        for (int e = 0; e < EPC; ++e) gw[e] = fmaf(dz, av[e], gw[e]);
        if (cl == 0) gb += dz;
        if (last) {
          // dA = sum over the output channels of dz[oc] * w[oc][c], summed in fp32 in channel order and rounded to the
          // storage type ONCE, on this last pass.  (Accumulating it through the stored tensor, one pass per output
          // channel, rounded every partial sum to bf16: an extra half bf16 ulp per output channel beyond the first.)
          const long n = pix[u] / HW, rem = pix[u] - n * HW;
#pragma unroll
          for (int e = 0; e < EPC; ++e) d[e] = 0.f;
          for (int o = 0; o < p.OC; ++o) {
            float dzo = dz;
            if (o != oc) {
              const long oo = (n * p.OC + o) * HW + rem;
              const float pro = p.probs[oo];
              dzo = p.dprobs[oo] * pro * (1.f - pro);
            }
#pragma unroll
            for (int e = 0; e < EPC; ++e) d[e] += dzo * (o == oc ? wv[e] : p.w[o * p.C + cl * EPC + e]);
          }
          if (dag) st16(dag + pix[u] * p.ldda + cl * EPC, Chunk<T>::pack(d));   // null: the consumer recomputes it (BnBwdParams::head_w)
        }
        if (BN && last) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) {
            const float g = round_through<T>(d[e]);
            const float gh = bn_dyhat(bn_nrm(yv[e], sc[e], sh[e]), g);
            const float xh = bn_xhat(yv[e], mu[e], rs[e]);
            bn_bwd_sums(gh, xh, s1[e], s2[e], s3[e]);
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) red[tid * (EPC + 1) + e] = gw[e];
    red[tid * (EPC + 1) + EPC] = gb;
    __syncthreads();
    for (int i = tid; i < p.C + 1; i += 256) {
      float s = 0.f;
      if (i < p.C) {
        const int c2 = i / EPC, e = i % EPC;
        for (int q = 0; q < ppb; ++q) s += red[(q * cpp + c2) * (EPC + 1) + e];
      } else {
        for (int q = 0; q < ppb; ++q) s += red[(q * cpp) * (EPC + 1) + EPC];
      }
      p.parts[((long)blockIdx.x * p.OC + oc) * (p.C + 1) + i] = s;
    }
    __syncthreads();
  }
  if (BN) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      red3[(tid * 3 + 0) * EPC + e] = s1[e];
      red3[(tid * 3 + 1) * EPC + e] = s2[e];
      red3[(tid * 3 + 2) * EPC + e] = s3[e];
    }
    __syncthreads();
    for (int i = tid; i < 3 * p.C; i += 256) {             // (which, channel): pixel lanes summed in lane order
      const int which = i / p.C, c = i - which * p.C, c2 = c / EPC, e = c - c2 * EPC;
      float s = 0.f;
      for (int q = 0; q < ppb; ++q) s += red3[((q * cpp + c2) * 3 + which) * EPC + e];
      p.bn_parts[((long)blockIdx.x * 3 + which) * p.C + c] = s;
    }
  }
}

__global__ __launch_bounds__(256) void head_bwd_finalize_kernel(const float* __restrict__ parts, int nparts, float* dw,
                                                                float* db, int OC, int C) {
  // 32 lanes per output element, rows l, l+32, ... each, fixed shuffle tree
  const int i = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
  const int L = OC * (C + 1);
  double s = 0.0;
  if (i < L)
    for (int q = l; q < nparts; q += 32) s += (double)parts[(long)q * L + i];
  s = lane32_sum(s);
  if (i >= L || l != 0) return;
  const int oc = i / (C + 1), c = i - oc * (C + 1);
  if (c < C) dw[oc * C + c] = (float)s;
  else db[oc] = (float)s;
}

HeadPlan plan_head(long P, int C, int OC, int dtype, long row_cap) {
  HeadPlan pl{};
  pl.epc = chunk_elems(dtype);
  if (!pl.epc || C <= 0 || C % pl.epc || OC < 1) return pl;
  pl.cpp = C / pl.epc;
  if (pl.cpp > 64 || (pl.cpp & (pl.cpp - 1))) return pl;
  pl.fwd_nb = grid_for(P, 4 * (256 / pl.cpp));                 // UNR = 4 pixels per lane group and trip
  const long per = (256 / pl.cpp) * 8, nb = (P + per - 1) / per, cap = row_cap < HEAD_BWD_MAX_ROWS ? row_cap : HEAD_BWD_MAX_ROWS;
  pl.bwd_nb = (int)(nb > cap ? cap : nb < 1 ? 1 : nb);        // >= 8 pixels per pixel lane
  pl.workspace = partial_floats(pl.bwd_nb, (long)OC * (C + 1)) * 4;
  pl.ok = true;
  return pl;
}

static int check_head(const HeadParams& p, const HeadPlan& pl, int dtype) {
  UNETDC_REQUIRE(pl.epc, "head: bad dtype %d", dtype);
  UNETDC_REQUIRE((p.a || p.bn_y) && p.w && p.probs, "head: null pointer");
  UNETDC_REQUIRE(p.lda % pl.epc == 0 && p.OC >= 1, "head: bad lda/OC");
  UNETDC_REQUIRE(pl.ok, "head: C=%d unsupported (C/%d must be a power of two <= 64)", p.C, pl.epc);
  return UNETDC_OK;
}

int launch_head_fwd(HeadParams& p, int dtype, hipStream_t stream) {
  const HeadPlan pl = plan_head((long)p.N * p.H * p.W, p.C, p.OC, dtype, HEAD_BWD_MAX_ROWS);
  int rc = check_head(p, pl, dtype);
  if (rc != UNETDC_OK) return rc;
  UNETDC_REQUIRE(p.b != nullptr, "head: null bias");
  const bool norm = p.bn_scale != nullptr;             // BatchNorm + ReLU of the producing stage applied on load
  if (norm) UNETDC_REQUIRE(p.bn_shift != nullptr, "head_fwd_bn: null shift");
  // C = 64 (the networks' head): 8 (bf16) / 16 (fp32) lanes per pixel known at compile time; other widths: generic form
  dispatch(dtype, [&](auto t, auto N, auto c64) {
    using T = typename decltype(t)::type;
    constexpr int CPP = decltype(c64)::value ? 64 / Chunk<T>::N : 0;
    hipLaunchKernelGGL((head_fwd_kernel<T, decltype(N)::value, CPP>), dim3(pl.fwd_nb), dim3(256), 0, stream, p);
  }, norm, p.C == 64);
  return check_launch("head_fwd_kernel");
}

int launch_head_bwd(HeadParams& p, float* dw, float* db, void* workspace, long workspace_bytes, int dtype,
                    hipStream_t stream, int* bn_nparts, long bn_parts_floats) {
  const bool bn = p.bn_y != nullptr;
  // bn: the caller sized bn_parts for a convolution epilogue (one row per 256 pixels + the spare rows): the grid-stride loop
  // of this kernel takes as many workgroups as that buffer has rows for
  const long cap = bn && p.C > 0 ? partial_row_cap(bn_parts_floats, 3L * p.C) : HEAD_BWD_MAX_ROWS;
  const HeadPlan pl = plan_head((long)p.N * p.H * p.W, p.C, p.OC, dtype, cap < 1 ? 1 : cap);
  int rc = check_head(p, pl, dtype);
  if (rc != UNETDC_OK) return rc;
  const int epc = pl.epc, nb = pl.bwd_nb;
  UNETDC_REQUIRE(p.dprobs && dw && db && workspace, "head_bwd: null pointer");
  // da == NULL: the gradient of the head's input is not stored (one output channel, fused BatchNorm-backward sums: the
  // stage's backward pass recomputes it, unetdc_bn_relu_bwd_head)
  UNETDC_REQUIRE(p.da || (p.OC == 1 && p.bn_y), "head_bwd: da may be NULL only with one output channel and the fused sums");
  UNETDC_REQUIRE(!p.da || p.ldda % epc == 0, "head_bwd: ldda not chunk aligned");
  UNETDC_REQUIRE(bn || p.a, "head_bwd: null activation");
  if (bn) {
    UNETDC_REQUIRE(p.bn_scale && p.bn_shift && p.bn_mean && p.bn_rstd && p.bn_parts && bn_nparts,
                   "head_bwd_bnstats: null pointer");
    UNETDC_REQUIRE(p.bn_ldy % epc == 0 && p.bn_ldy >= p.C, "head_bwd_bnstats: ldy not chunk aligned");
    UNETDC_REQUIRE(cap >= 1, "head_bwd_bnstats: partial buffer too small");
    *bn_nparts = nb;
  }
  if (pl.workspace > workspace_bytes) {
    set_error("head_bwd: workspace too small (%ld < %ld bytes)", workspace_bytes, pl.workspace);
    return UNETDC_EWORKSPACE;
  }
  p.parts = reinterpret_cast<float*>(workspace);
  dispatch(dtype, [&](auto t, auto B, auto Ln) {
    using T = typename decltype(t)::type;
    constexpr bool BN = decltype(B)::value, LEAN = decltype(Ln)::value;
    if constexpr (!LEAN || BN) hipLaunchKernelGGL((head_bwd_kernel<T, BN, LEAN>), dim3(nb), dim3(256), 0, stream, p);
  }, bn, bn && !p.a && !p.da && p.OC == 1);
  rc = check_launch("head_bwd_kernel");
  if (rc != UNETDC_OK) return rc;
  const int L = p.OC * (p.C + 1);
  const float* rp; int rows;
  rc = reduce_parts(p.parts, nb, L, &rp, &rows, stream, REDUCE_DIRECT);
  if (rc != UNETDC_OK) return rc;
  hipLaunchKernelGGL(head_bwd_finalize_kernel, dim3((L + 7) / 8), dim3(256), 0, stream, rp, rows, dw, db, p.OC, p.C);
  return check_launch("head_bwd_finalize_kernel");
}

}  // namespace unetdc
