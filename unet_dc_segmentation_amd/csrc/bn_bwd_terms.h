// The BatchNorm + ReLU backward arithmetic per element, stated once for bn_bwd_kernel (two sites, batchnorm.hip) and
// head_bwd_kernel (two, head.hip): the exact tests need the sites to agree to the bit.  first_wgrad_rows_kernel (first_conv.hip)
// keeps the same operations written out: through these helpers its bf16 form was scheduled differently and measured 0.7 %
// slower (profiles/elementwise_refactor_ab.txt).  y: saved conv output, nrm = scale * y + shift, g: gradient of the activation.
#pragma once
#include "common.h"

namespace unetdc {

__device__ __forceinline__ float bn_nrm(float y, float sc, float sh) { return fmaf(y, sc, sh); }
__device__ __forceinline__ float bn_dyhat(float nrm, float g) { return nrm > 0.f ? g : 0.f; }        // gh = g * [a > 0]
__device__ __forceinline__ float bn_xhat(float y, float mu, float rs) { return (y - mu) * rs; }     // xh
// S1 = sum dyhat, S2 = sum dyhat * xhat, S3 = sum xhat
__device__ __forceinline__ void bn_bwd_sums(float gh, float xh, float& s1, float& s2, float& s3) {
  s1 += gh; s2 = fmaf(gh, xh, s2); s3 += xh;
}
// dy = k1 * dyhat - k2 - k3 * xhat
__device__ __forceinline__ float bn_bwd_apply(float k1, float k2, float k3, float gh, float xh) {
  return fmaf(k1, gh, -k2) - k3 * xh;
}

}  // namespace unetdc
