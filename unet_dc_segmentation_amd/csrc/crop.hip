// Training at native resolution: random S x S windows of images cached at their OWN size as HWC uint8,
// cut, scaled to [0, 1] and augmented in one pass.  The rule is stated once in utils/crops.py; crop_gather_numpy there is
// this kernel on the host.
//
//   window   win[c][y][x] = float(img[fold(y0 + y, h)][fold(x0 + x, w)][c]) / 255.0f, mwin[y][x] = mask[same pixel]; fold is
//            the reflect-101 rule of tile.hip (utils/tiling.py:fold).  Only an image smaller than S along an axis is ever
//            folded, and its origin on that axis is 0.
//   output   the random part of TrainAugment applied to the window AS IF IT WERE THE IMAGE: gather_pixel (gather_index.h), the
//            one body augment_gather_kernel runs too, on the S x S lattice (index permutation, per-tap brightness / contrast,
//            four bilinear taps and a nearest mask tap, reflected at the WINDOW's border) with the window lookup as its lattice.
//
// One thread per output pixel, all channels and the mask.  Records go BY VALUE in the launch arguments (AUG_MAX_BATCH per
// launch): the host writes no device memory per batch, nothing waits on the device, no workspace, no atomics.  Every
// coordinate is folded into its image, so every read lies inside the image of its record for any accepted record.
//
// Two kernels, one record (CropRecord) and one launcher: crop_gather_kernel reads the window pixel itself,
// crop_gather_scaled_kernel (below) resamples a T x T source window to the lattice.
#include "gather_index.h"
#include "kernels.h"
#include "linear_u8.h"

namespace unetdc {

constexpr int CROP_MIN_S = 16, CROP_MAX_S = 1024;    // 1024: the largest side of an elastic field (augment.hip AUG_MAX_SIDE)
constexpr int CROP_MAX_SIDE = 16384;

struct CropBatch {
  CropRecord r[AUG_MAX_BATCH];              // 32 x 56 = 1792 bytes by value, well inside the 4 KB of launch arguments
};

// pixel offset (from the image's first) of window pixel (wy, wx) in the HWC image of record p
__device__ inline long crop_pixel(const CropRecord& p, int wy, int wx) {
  return (long)tile_fold(p.y0 + wy, p.h) * p.w + tile_fold(p.x0 + wx, p.w);
}

// The folded S x S window as a lattice of gather_pixel (gather_index.h): a byte of the HWC image, scaled to [0, 1]
struct WindowLattice {
  const unsigned char* img;
  const unsigned char* msk;
  const CropRecord& p;
  int C;
  __device__ __forceinline__ long tap(int sy, int sx) const { return crop_pixel(p, sy, sx); }
  __device__ __forceinline__ float value(long s, int c) const { return (float)img[s * C + c] / 255.0f; }
  __device__ __forceinline__ float mask(int sy, int sx) const { return (float)msk[crop_pixel(p, sy, sx)]; }
};

// grid (S / 16, S / 16, n), block 16 x 16: thread = output pixel (y, x) of sample n0 + blockIdx.z.  out_img [N][C][S][S] fp32,
// out_mask [N][1][S][S] fp32.
__global__ __launch_bounds__(256) void crop_gather_kernel(const unsigned char* __restrict__ images,
                                                          const unsigned char* __restrict__ masks, int C, int S,
                                                          const float* __restrict__ fields, const CropBatch b, int n0,
                                                          float* __restrict__ out_img, float* __restrict__ out_mask) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= S || y >= S) return;
  const CropRecord& p = b.r[blockIdx.z];
  const long ss = (long)S * S, pix = (long)y * S + x, n = n0 + blockIdx.z;
  const WindowLattice L{images + p.img_off, masks + p.mask_off, p, C};
  gather_pixel(L, p, C, S, S, y, x, fields, out_img + n * C * ss + pix, out_mask + n * ss + pix);
}

// ---- scale jitter (--crop_scale, --crop_fg): a T x T source window resampled to the S x S lattice in the same pass ----------------
//
//   lattice  L[c][y][x] = float(R[y][x][c]) / 255.0f, where R = utils.data_loader.resize_linear_cv2_u8(source window, S, S): OpenCV's
//            8-bit INTER_LINEAR.  Per lattice coordinate d the taps of linear_tables(T, S): f = (d + 0.5) * (T / S) - 0.5 in
//            double (product and subtraction rounded apart), first tap floor(f), coefficients rint((1.0f - float(frac)) * 2048)
//            and rint(float(frac) * 2048).  The border rules differ per axis, as that function has them -- x: a first tap left
//            of pixel 0 or at / past pixel T - 1 becomes ONE tap of weight 2048; y: two taps, each clamped to 0..T-1, weights
//            kept -- so the resize acts in the window's own orientation, before any flip or rotation.  Then the integer passes
//            of linear_u8_combine (linear_u8.h).  The mask lattice is the source mask at min(floor(d * (T / S)), T - 1) on both
//            axes (INTER_NEAREST).
//   output   gather_pixel on that lattice.  At T == S every coefficient pair is (2048, 0), v is the pixel itself and the two
//            kernels agree bit for bit.
//
// The tap arithmetic is a handful of fp64 operations per lattice tap (2 per plain pixel, 8 with a field) next to 4 source bytes
// per channel and tap and the 16 bytes a thread writes (three channels and the mask, float32).  Every tap index is clamped to the
// source window and then folded into the image, so every read of an accepted record lies inside its image.

// the two taps (window coordinates, clamped) and 11-bit coefficients of lattice coordinate d along one axis
template <bool IS_X>
__device__ __forceinline__ void crop_scaled_taps(int d, int T, double scale, int& i0, int& i1, int& a0, int& a1) {
  double m = ((double)d + 0.5) * scale;
  asm volatile("" : "+v"(m));                               // the product is rounded before the subtraction (no FMA), as numpy
  double f = m - 0.5;
  const double fl = floor(f);
  const int s = (int)fl;
  const float fr = (float)(f - fl);
  a0 = (int)rintf((1.0f - fr) * 2048.0f);
  a1 = (int)rintf(fr * 2048.0f);
  if (IS_X) {
    if (s < 0 || s >= T - 1) { a0 = 2048; a1 = 0; }
    i0 = min(max(s, 0), T - 1);
    i1 = min(i0 + 1, T - 1);
  } else {
    i0 = min(max(s, 0), T - 1);
    i1 = min(max(s + 1, 0), T - 1);
  }
}

// One lattice pixel: offsets (in pixels, from the image's first) of its four source pixels, and its coefficients
struct ScaledTap {
  int s00, s01, s10, s11, a0, a1, b0, b1;
};

__device__ __forceinline__ ScaledTap crop_scaled_tap(const CropRecord& p, double scale, int ly, int lx) {
  ScaledTap t;
  int y0, y1, x0, x1;
  crop_scaled_taps<false>(ly, p.t, scale, y0, y1, t.b0, t.b1);
  crop_scaled_taps<true>(lx, p.t, scale, x0, x1, t.a0, t.a1);
  const int r0 = tile_fold(p.y0 + y0, p.h) * p.w, r1 = tile_fold(p.y0 + y1, p.h) * p.w;      // h * w <= 2^28
  const int c0 = tile_fold(p.x0 + x0, p.w), c1 = tile_fold(p.x0 + x1, p.w);
  t.s00 = r0 + c0; t.s01 = r0 + c1; t.s10 = r1 + c0; t.s11 = r1 + c1;
  return t;
}

__device__ __forceinline__ float crop_scaled_value(const unsigned char* __restrict__ img, const ScaledTap& t, int C, int c) {
  const int v = linear_u8_combine(img[t.s00 * C + c], img[t.s01 * C + c], img[t.s10 * C + c], img[t.s11 * C + c], t.a0, t.a1,
                                  t.b0, t.b1);
  return (float)min(max(v, 0), 255) / 255.0f;
}

// the mask byte of lattice pixel (ly, lx): the nearest source pixel
__device__ __forceinline__ float crop_scaled_mask(const unsigned char* __restrict__ msk, const CropRecord& p, double scale,
                                                  int ly, int lx) {
  const int wy = min((int)floor((double)ly * scale), p.t - 1), wx = min((int)floor((double)lx * scale), p.t - 1);
  return (float)msk[(long)tile_fold(p.y0 + wy, p.h) * p.w + tile_fold(p.x0 + wx, p.w)];
}

// The T x T source window resampled to S x S as a lattice of gather_pixel
struct ScaledLattice {
  const unsigned char* img;
  const unsigned char* msk;
  const CropRecord& p;
  int C;
  double scale;                             // T / S
  __device__ __forceinline__ ScaledTap tap(int sy, int sx) const { return crop_scaled_tap(p, scale, sy, sx); }
  __device__ __forceinline__ float value(const ScaledTap& t, int c) const { return crop_scaled_value(img, t, C, c); }
  __device__ __forceinline__ float mask(int sy, int sx) const { return crop_scaled_mask(msk, p, scale, sy, sx); }
};

// grid and outputs as crop_gather_kernel
__global__ __launch_bounds__(256) void crop_gather_scaled_kernel(const unsigned char* __restrict__ images,
                                                                 const unsigned char* __restrict__ masks, int C, int S,
                                                                 const float* __restrict__ fields, const CropBatch b, int n0,
                                                                 float* __restrict__ out_img, float* __restrict__ out_mask) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= S || y >= S) return;
  const CropRecord& p = b.r[blockIdx.z];
  const long ss = (long)S * S, pix = (long)y * S + x, n = n0 + blockIdx.z;
  const ScaledLattice L{images + p.img_off, masks + p.mask_off, p, C, (double)p.t / (double)S};
  gather_pixel(L, p, C, S, S, y, x, fields, out_img + n * C * ss + pix, out_mask + n * ss + pix);
}

// Both crop entry points.  who: the entry point's name for the messages; scaled: the source window of record i has side
// params[i].t (checked against s / 2 .. 2 s), else side s and t is not read.
int launch_crop_gather(const char* who, bool scaled, const unsigned char* images, long images_bytes, const unsigned char* masks,
                       long masks_bytes, int c, int s, const CropRecord* params, int n, const float* fields, int nfields,
                       float* out_img, float* out_mask, hipStream_t stream) {
  UNETDC_REQUIRE(images && masks && params && out_img && out_mask, "%s: null pointer", who);
  UNETDC_REQUIRE(s % 16 == 0 && s >= CROP_MIN_S && s <= CROP_MAX_S, "%s: crop size %d outside the limits (a multiple of 16 in %d..%d)",
                 who, s, CROP_MIN_S, CROP_MAX_S);
  UNETDC_REQUIRE(c >= 1 && c <= 4 && n >= 0 && nfields >= 0 && images_bytes >= 0 && masks_bytes >= 0,
                 "%s: bad geometry c=%d n=%d nfields=%d (channels 1..4)", who, c, n, nfields);
  for (int i = 0; i < n; ++i) {
    const CropRecord& p = params[i];
    UNETDC_REQUIRE(p.h >= 1 && p.w >= 1 && p.h <= CROP_MAX_SIDE && p.w <= CROP_MAX_SIDE,
                   "%s: sample %d: image of %d x %d (sides 1..%d)", who, i, p.h, p.w, CROP_MAX_SIDE);
    UNETDC_REQUIRE(!scaled || (p.t >= s / 2 && p.t <= 2 * s), "%s: sample %d: source side %d outside %d..%d", who, i, p.t, s / 2,
                   2 * s);
    const int t = scaled ? p.t : s;
    const int ymax = p.h > t ? p.h - t : 0, xmax = p.w > t ? p.w - t : 0;
    UNETDC_REQUIRE(p.y0 >= 0 && p.y0 <= ymax && p.x0 >= 0 && p.x0 <= xmax, "%s: sample %d: origin (%d, %d) outside 0..%d, 0..%d",
                   who, i, p.y0, p.x0, ymax, xmax);
    const long long hw = (long long)p.h * p.w;
    UNETDC_REQUIRE(p.img_off >= 0 && p.img_off <= images_bytes && hw * c <= images_bytes - p.img_off,
                   "%s: sample %d: image at offset %lld leaves the buffer of %ld bytes", who, i, p.img_off, images_bytes);
    UNETDC_REQUIRE(p.mask_off >= 0 && p.mask_off <= masks_bytes && hw <= masks_bytes - p.mask_off,
                   "%s: sample %d: mask at offset %lld leaves the buffer of %ld bytes", who, i, p.mask_off, masks_bytes);
    if (const int rc = check_gather_record(who, i, p, fields, nfields)) return rc;
  }
  for_gather_batches<CropBatch>(params, n, [&](const CropBatch& b, int m, int n0) {
    hipLaunchKernelGGL(scaled ? crop_gather_scaled_kernel : crop_gather_kernel, dim3(s / 16, s / 16, m), dim3(256), 0, stream,
                       images, masks, c, s, fields, b, n0, out_img, out_mask);
  });
  return n ? check_launch(scaled ? "crop_gather_scaled_kernel" : "crop_gather_kernel") : UNETDC_OK;
}

}  // namespace unetdc
