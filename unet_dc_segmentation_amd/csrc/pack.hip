// Weight packing (fp32 PyTorch layouts -> K-contiguous "[tap][out][in]" images in the compute type)
#include "kernels.h"

namespace unetdc {

template <typename T>
__global__ void pack_conv3x3_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wd, int Co, int Ci) {
  const long n = (long)Co * Ci * 9;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    // i indexes the forward image [t][co][ci]
    const int ci = (int)(i % Ci);
    const long r = i / Ci;
    const int co = (int)(r % Co), t = (int)(r / Co);
    const float v = w[((long)co * Ci + ci) * 9 + t];
    wf[i] = from_f32<T>(v);
    // dgrad image [t'][ci][co] with t' = 8 - t (both spatial axes flipped)
    if (wd) wd[((long)(8 - t) * Ci + ci) * Co + co] = from_f32<T>(v);
  }
}

int launch_pack_conv3x3(const float* w, void* wf, void* wd, int Co, int Ci, int dtype, hipStream_t stream) {
  UNETDC_REQUIRE(w && wf, "pack_conv3x3: null pointer");
  UNETDC_REQUIRE(chunk_elems(dtype), "pack_conv3x3: bad dtype %d", dtype);
  dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pack_conv3x3_kernel<T>, dim3(grid_for((long)Co * Ci * 9, 256)), dim3(256), 0, stream, w, (T*)wf, (T*)wd, Co, Ci);
  });
  return check_launch("pack_conv3x3_kernel");
}

template <typename T>
__global__ void pack_convT2x2_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wd, int Ci, int Co) {
  const long n = (long)Ci * Co * 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    // i indexes the forward image [(ab)*Co + co][ci]
    const int ci = (int)(i % Ci);
    const long r = i / Ci;
    const int co = (int)(r % Co), ab = (int)(r / Co);
    const float v = w[((long)ci * Co + co) * 4 + ab];
    wf[i] = from_f32<T>(v);
    if (wd) wd[((long)ab * Ci + ci) * Co + co] = from_f32<T>(v);    // dgrad image [ab][ci][co]
  }
}

int launch_pack_convT2x2(const float* w, void* wf, void* wd, int Ci, int Co, int dtype, hipStream_t stream) {
  UNETDC_REQUIRE(w && wf, "pack_convT2x2: null pointer");
  UNETDC_REQUIRE(chunk_elems(dtype), "pack_convT2x2: bad dtype %d", dtype);
  dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pack_convT2x2_kernel<T>, dim3(grid_for((long)Co * Ci * 4, 256)), dim3(256), 0, stream, w, (T*)wf, (T*)wd, Ci, Co);
  });
  return check_launch("pack_convT2x2_kernel");
}

// All layers in ONE launch, as an LDS-tiled transpose: a device-resident table describes each tensor
// (21 per network); one workgroup handles a 32 x 32 (out x in) channel tile with all its taps, reads
// the fp32 parameter in contiguous 1152/512-byte rows and writes both K-contiguous images in >= 64-byte
// runs.  (Element-wise scattering of the transposed dgrad image cost 0.3 ms per step.)
struct PackDesc {
  const float* w;      // fp32 parameter, PyTorch layout
  void* wf;            // forward image
  void* wd;            // dgrad image (nullable)
  long begin;          // index of this tensor's first 32x32 tile in the launch
  int a, b;            // conv3x3: (Cout, Cin), taps 9;  convT: (Cin, Cout), taps 4
  int kind;            // 0 = conv3x3, 1 = convT2x2
  int pad;
};

template <typename T>
__global__ __launch_bounds__(256) void pack_many_kernel(const PackDesc* __restrict__ table, int n) {
  __shared__ float tile[32 * 289];
  const int tid = threadIdx.x;
  const long tix = blockIdx.x;
  int lo = 0, hi = n - 1;                      // last descriptor with begin <= tix
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].begin <= tix) lo = mid; else hi = mid - 1;
  }
  const PackDesc d = table[lo];
  const int local = (int)(tix - d.begin);
  T* wf = reinterpret_cast<T*>(d.wf);
  T* wd = reinterpret_cast<T*>(d.wd);
  if (d.kind == 0) {
    const int Co = d.a, Ci = d.b, tci = Ci / 32;
    const int co0 = (local / tci) * 32, ci0 = (local % tci) * 32;
    for (int i = tid; i < 32 * 288; i += 256) {            // w[co][ci0 .. ci0+31][9]: 288 contiguous floats
      const int co = i / 288, rem = i - co * 288;
      tile[co * 289 + rem] = d.w[((long)(co0 + co) * Ci + ci0) * 9 + rem];
    }
    __syncthreads();
    for (int i = tid; i < 9 * 1024; i += 256) {
      const int t = i >> 10, x = (i >> 5) & 31, y = i & 31;
      wf[((long)t * Co + co0 + x) * Ci + ci0 + y] = from_f32<T>(tile[x * 289 + y * 9 + t]);            // x = co, y = ci
      if (wd) wd[((long)(8 - t) * Ci + ci0 + x) * Co + co0 + y] = from_f32<T>(tile[y * 289 + x * 9 + t]);  // x = ci, y = co
    }
  } else {
    const int Ci = d.a, Co = d.b, tco = Co / 32;
    const int ci0 = (local / tco) * 32, co0 = (local % tco) * 32;
    for (int i = tid; i < 32 * 128; i += 256) {            // w[ci][co0 .. co0+31][4]: 128 contiguous floats
      const int ci = i >> 7, rem = i & 127;
      tile[ci * 129 + rem] = d.w[((long)(ci0 + ci) * Co + co0) * 4 + rem];
    }
    __syncthreads();
    for (int i = tid; i < 4 * 1024; i += 256) {
      const int ab = i >> 10, x = (i >> 5) & 31, y = i & 31;
      wf[((long)ab * Co + co0 + x) * Ci + ci0 + y] = from_f32<T>(tile[y * 129 + x * 4 + ab]);              // x = co, y = ci
      if (wd) wd[((long)ab * Ci + ci0 + x) * Co + co0 + y] = from_f32<T>(tile[x * 129 + y * 4 + ab]);        // x = ci, y = co
    }
  }
}

int launch_pack_many(const void* table_dev, int n, long total_tiles, int dtype, hipStream_t stream) {
  UNETDC_REQUIRE(table_dev && n > 0 && total_tiles > 0 && total_tiles < (1L << 31), "pack_many: empty table");
  UNETDC_REQUIRE(chunk_elems(dtype), "pack_many: bad dtype %d", dtype);
  dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pack_many_kernel<T>, dim3((unsigned)total_tiles), dim3(256), 0, stream, reinterpret_cast<const PackDesc*>(table_dev), n);
  });
  return check_launch("pack_many_kernel");
}

}  // namespace unetdc
