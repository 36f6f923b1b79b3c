// The 32-bit finaliser behind the counter-based hashes of augment.hip (elastic noise) and spatial.hip (simulated point patterns).
#pragma once
#include <hip/hip_runtime.h>

namespace unetdc {

__host__ __device__ inline unsigned aug_fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

}  // namespace unetdc
