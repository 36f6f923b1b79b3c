// Training at native resolution: random S x S windows of images cached at their OWN size as HWC uint8,
// cut, scaled to [0, 1] and augmented in one pass.  The rule is stated once in utils/crops.py; crop_gather_numpy there is
// this kernel on the host.
//
//   window   win[c][y][x] = float(img[fold(y0 + y, h)][fold(x0 + x, w)][c]) / 255.0f, mwin[y][x] = mask[same pixel]; fold is
//            the reflect-101 rule of tile.hip (utils/tiling.py:fold).  Only an image smaller than S along an axis is ever
//            folded, and its origin on that axis is 0.
//   output   the random part of TrainAugment applied to the window AS IF IT WERE THE IMAGE: augment_gather_kernel on the S x S
//            lattice (same index permutation, same per-tap brightness / contrast, same four bilinear taps and nearest mask tap,
//            reflected at the WINDOW's border) with the window lookup in place of the cache read.
//
// One thread per output pixel, all channels and the mask.  Records go BY VALUE in the launch arguments (AUG_MAX_BATCH per
// launch): the host writes no device memory per batch, nothing waits on the device, no workspace, no atomics.  Every
// coordinate is folded into its image, so every read lies inside the image of its record for any accepted record.
#include "gather_index.h"
#include "kernels.h"

namespace unetdc {

constexpr int CROP_MIN_S = 16, CROP_MAX_S = 1024;    // 1024: the largest side of an elastic field (augment.hip AUG_MAX_SIDE)
constexpr int CROP_MAX_SIDE = 16384;

struct CropBatch {
  CropRecord r[AUG_MAX_BATCH];
};

// byte offset of channel 0 of window pixel (wy, wx) in the HWC image of record p
__device__ inline long crop_pixel(const CropRecord& p, int wy, int wx) {
  return (long)tile_fold(p.y0 + wy, p.h) * p.w + tile_fold(p.x0 + wx, p.w);
}

// grid (S / 16, S / 16, n), block 16 x 16: thread = output pixel (y, x) of sample n0 + blockIdx.z.  out_img [N][C][S][S] fp32,
// out_mask [N][1][S][S] fp32.
__global__ __launch_bounds__(256) void crop_gather_kernel(const unsigned char* __restrict__ images,
                                                          const unsigned char* __restrict__ masks, int C, int S,
                                                          const float* __restrict__ fields, const CropBatch b, int n0,
                                                          float* __restrict__ out_img, float* __restrict__ out_mask) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= S || y >= S) return;
  const CropRecord& p = b.r[blockIdx.z];
  const long ss = (long)S * S, pix = (long)y * S + x;
  const unsigned char* img = images + p.img_off;
  const unsigned char* msk = masks + p.mask_off;
  const long n = n0 + blockIdx.z;
  float* oi = out_img + n * C * ss + pix;
  if (p.field < 0) {
    int sy, sx;
    aug_source(y, x, S, S, p.flags, p.k, sy, sx);
    const long s = crop_pixel(p, sy, sx);
    for (int c = 0; c < C; ++c) oi[c * ss] = aug_bc((float)img[s * C + c] / 255.0f, p);
    out_mask[n * ss + pix] = (float)msk[s];
    return;
  }
  const float* f = fields + (long)p.field * 2 * ss;
  const float dx = f[pix], dy = f[ss + pix];
  const float fx = floorf(dx), fy = floorf(dy);
  const float tx = dx - fx, ty = dy - fy;                   // exact: the fraction of a float32
  const int ix = x + (int)fx, iy = y + (int)fy;
  int sy, sx;
  long s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    aug_source(aug_reflect(iy + (q >> 1), S), aug_reflect(ix + (q & 1), S), S, S, p.flags, p.k, sy, sx);
    s[q] = crop_pixel(p, sy, sx) * C;
  }
  const float wx0 = 1.0f - tx, wy0 = 1.0f - ty;
  for (int c = 0; c < C; ++c) {
    const float a00 = aug_bc((float)img[s[0] + c] / 255.0f, p), a01 = aug_bc((float)img[s[1] + c] / 255.0f, p);
    const float a10 = aug_bc((float)img[s[2] + c] / 255.0f, p), a11 = aug_bc((float)img[s[3] + c] / 255.0f, p);
    oi[c * ss] = wy0 * (wx0 * a00 + tx * a01) + ty * (wx0 * a10 + tx * a11);
  }
  // order 0: the nearest tap, round half up (ties are measure-zero for a smooth float field)
  aug_source(aug_reflect(iy + (ty >= 0.5f), S), aug_reflect(ix + (tx >= 0.5f), S), S, S, p.flags, p.k, sy, sx);
  out_mask[n * ss + pix] = (float)msk[crop_pixel(p, sy, sx)];
}

int launch_crop_gather(const unsigned char* images, long images_bytes, const unsigned char* masks, long masks_bytes, int c, int s,
                       const CropRecord* params, int n, const float* fields, int nfields, float* out_img, float* out_mask,
                       hipStream_t stream) {
  UNETDC_REQUIRE(images && masks && params && out_img && out_mask, "crop_gather: null pointer");
  UNETDC_REQUIRE(s % 16 == 0 && s >= CROP_MIN_S && s <= CROP_MAX_S, "crop_gather: crop size %d outside the limits (a multiple of 16 in %d..%d)",
                 s, CROP_MIN_S, CROP_MAX_S);
  UNETDC_REQUIRE(c >= 1 && c <= 4 && n >= 0 && nfields >= 0 && images_bytes >= 0 && masks_bytes >= 0,
                 "crop_gather: bad geometry c=%d n=%d nfields=%d (channels 1..4)", c, n, nfields);
  for (int i = 0; i < n; ++i) {
    const CropRecord& p = params[i];
    UNETDC_REQUIRE(p.h >= 1 && p.w >= 1 && p.h <= CROP_MAX_SIDE && p.w <= CROP_MAX_SIDE,
                   "crop_gather: sample %d: image of %d x %d (sides 1..%d)", i, p.h, p.w, CROP_MAX_SIDE);
    const int ymax = p.h > s ? p.h - s : 0, xmax = p.w > s ? p.w - s : 0;
    UNETDC_REQUIRE(p.y0 >= 0 && p.y0 <= ymax && p.x0 >= 0 && p.x0 <= xmax,
                   "crop_gather: sample %d: origin (%d, %d) outside 0..%d, 0..%d", i, p.y0, p.x0, ymax, xmax);
    const long long hw = (long long)p.h * p.w;
    UNETDC_REQUIRE(p.img_off >= 0 && p.img_off <= images_bytes && hw * c <= images_bytes - p.img_off,
                   "crop_gather: sample %d: image at offset %lld leaves the buffer of %ld bytes", i, p.img_off, images_bytes);
    UNETDC_REQUIRE(p.mask_off >= 0 && p.mask_off <= masks_bytes && hw <= masks_bytes - p.mask_off,
                   "crop_gather: sample %d: mask at offset %lld leaves the buffer of %ld bytes", i, p.mask_off, masks_bytes);
    UNETDC_REQUIRE(p.k >= 0 && p.k <= 3, "crop_gather: sample %d: k = %d (0..3)", i, p.k);
    UNETDC_REQUIRE((p.flags & ~(AUG_HFLIP | AUG_VFLIP | AUG_BC)) == 0, "crop_gather: sample %d: bad flags 0x%x", i, p.flags);
    UNETDC_REQUIRE(p.field >= -1 && p.field < nfields, "crop_gather: sample %d: field slot %d outside [-1, %d)", i, p.field,
                   nfields);
    UNETDC_REQUIRE(p.field < 0 || fields, "crop_gather: sample %d draws elastic but fields is null", i);
  }
  for (int s0 = 0; s0 < n; s0 += AUG_MAX_BATCH) {
    const int m = n - s0 < AUG_MAX_BATCH ? n - s0 : AUG_MAX_BATCH;
    CropBatch b = {};
    for (int i = 0; i < m; ++i) b.r[i] = params[s0 + i];
    hipLaunchKernelGGL(crop_gather_kernel, dim3(s / 16, s / 16, m), dim3(256), 0, stream, images, masks, c, s, fields, b, s0,
                       out_img, out_mask);
  }
  return n ? check_launch("crop_gather_kernel") : UNETDC_OK;
}

// ---- scale jitter (--crop_scale, --crop_fg): a T x T source window resampled to the S x S lattice in the same pass ----------------
//
//   lattice  L[c][y][x] = float(R[y][x][c]) / 255.0f, where R = utils.data_loader.resize_linear_cv2_u8(source window, S, S): OpenCV's
//            8-bit INTER_LINEAR.  Per lattice coordinate d the taps of linear_tables(T, S): f = (d + 0.5) * (T / S) - 0.5 in
//            double (product and subtraction rounded apart), first tap floor(f), coefficients rint((1.0f - float(frac)) * 2048)
//            and rint(float(frac) * 2048).  The border rules differ per axis, as that function has them -- x: a first tap left
//            of pixel 0 or at / past pixel T - 1 becomes ONE tap of weight 2048; y: two taps, each clamped to 0..T-1, weights
//            kept -- so the resize acts in the window's own orientation, before any flip or rotation.  Then the integer passes
//            r = p0 * a0 + p1 * a1 per row, v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.  The mask lattice
//            is the source mask at min(floor(d * (T / S)), T - 1) on both axes (INTER_NEAREST).
//   output   crop_gather_kernel on that lattice.  At T == S every coefficient pair is (2048, 0), v is the pixel itself and the
//            two kernels agree bit for bit.
//
// The tap arithmetic is a handful of fp64 operations per lattice tap (2 per plain pixel, 8 with a field) next to 4 source bytes
// per channel and tap and the 16 bytes a thread writes (three channels and the mask, float32).  Every tap index is clamped to the
// source window and then folded into the image, so every read of an accepted record lies inside its image.
struct CropScaledBatch {
  CropScaledRecord r[AUG_MAX_BATCH];        // 32 x 56 = 1792 bytes by value, well inside the 4 KB of launch arguments
};

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

__device__ __forceinline__ ScaledTap crop_scaled_tap(const CropScaledRecord& p, double scale, int ly, int lx) {
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
  const int r0 = (int)img[t.s00 * C + c] * t.a0 + (int)img[t.s01 * C + c] * t.a1;
  const int r1 = (int)img[t.s10 * C + c] * t.a0 + (int)img[t.s11 * C + c] * t.a1;
  int v = (((t.b0 * (r0 >> 4)) >> 16) + ((t.b1 * (r1 >> 4)) >> 16) + 2) >> 2;
  v = min(max(v, 0), 255);
  return (float)v / 255.0f;
}

// the mask byte of lattice pixel (ly, lx): the nearest source pixel
__device__ __forceinline__ float crop_scaled_mask(const unsigned char* __restrict__ msk, const CropScaledRecord& p, double scale,
                                                  int ly, int lx) {
  const int wy = min((int)floor((double)ly * scale), p.t - 1), wx = min((int)floor((double)lx * scale), p.t - 1);
  return (float)msk[(long)tile_fold(p.y0 + wy, p.h) * p.w + tile_fold(p.x0 + wx, p.w)];
}

// grid and outputs as crop_gather_kernel
__global__ __launch_bounds__(256) void crop_gather_scaled_kernel(const unsigned char* __restrict__ images,
                                                                 const unsigned char* __restrict__ masks, int C, int S,
                                                                 const float* __restrict__ fields, const CropScaledBatch b,
                                                                 int n0, float* __restrict__ out_img,
                                                                 float* __restrict__ out_mask) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= S || y >= S) return;
  const CropScaledRecord& p = b.r[blockIdx.z];
  const long ss = (long)S * S, pix = (long)y * S + x;
  const unsigned char* img = images + p.img_off;
  const unsigned char* msk = masks + p.mask_off;
  const long n = n0 + blockIdx.z;
  const double scale = (double)p.t / (double)S;
  float* oi = out_img + n * C * ss + pix;
  if (p.field < 0) {
    int sy, sx;
    aug_source(y, x, S, S, p.flags, p.k, sy, sx);
    const ScaledTap t = crop_scaled_tap(p, scale, sy, sx);
    for (int c = 0; c < C; ++c) oi[c * ss] = aug_bc(crop_scaled_value(img, t, C, c), p);
    out_mask[n * ss + pix] = crop_scaled_mask(msk, p, scale, sy, sx);
    return;
  }
  const float* f = fields + (long)p.field * 2 * ss;
  const float dx = f[pix], dy = f[ss + pix];
  const float fx = floorf(dx), fy = floorf(dy);
  const float tx = dx - fx, ty = dy - fy;                   // exact: the fraction of a float32
  const int ix = x + (int)fx, iy = y + (int)fy;
  int sy, sx;
  ScaledTap t[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    aug_source(aug_reflect(iy + (q >> 1), S), aug_reflect(ix + (q & 1), S), S, S, p.flags, p.k, sy, sx);
    t[q] = crop_scaled_tap(p, scale, sy, sx);
  }
  const float wx0 = 1.0f - tx, wy0 = 1.0f - ty;
  for (int c = 0; c < C; ++c) {
    const float a00 = aug_bc(crop_scaled_value(img, t[0], C, c), p), a01 = aug_bc(crop_scaled_value(img, t[1], C, c), p);
    const float a10 = aug_bc(crop_scaled_value(img, t[2], C, c), p), a11 = aug_bc(crop_scaled_value(img, t[3], C, c), p);
    oi[c * ss] = wy0 * (wx0 * a00 + tx * a01) + ty * (wx0 * a10 + tx * a11);
  }
  aug_source(aug_reflect(iy + (ty >= 0.5f), S), aug_reflect(ix + (tx >= 0.5f), S), S, S, p.flags, p.k, sy, sx);
  out_mask[n * ss + pix] = crop_scaled_mask(msk, p, scale, sy, sx);
}

int launch_crop_gather_scaled(const unsigned char* images, long images_bytes, const unsigned char* masks, long masks_bytes, int c,
                              int s, const CropScaledRecord* params, int n, const float* fields, int nfields, float* out_img,
                              float* out_mask, hipStream_t stream) {
  UNETDC_REQUIRE(images && masks && params && out_img && out_mask, "crop_gather_scaled: null pointer");
  UNETDC_REQUIRE(s % 16 == 0 && s >= CROP_MIN_S && s <= CROP_MAX_S,
                 "crop_gather_scaled: crop size %d outside the limits (a multiple of 16 in %d..%d)", s, CROP_MIN_S, CROP_MAX_S);
  UNETDC_REQUIRE(c >= 1 && c <= 4 && n >= 0 && nfields >= 0 && images_bytes >= 0 && masks_bytes >= 0,
                 "crop_gather_scaled: bad geometry c=%d n=%d nfields=%d (channels 1..4)", c, n, nfields);
  for (int i = 0; i < n; ++i) {
    const CropScaledRecord& p = params[i];
    UNETDC_REQUIRE(p.h >= 1 && p.w >= 1 && p.h <= CROP_MAX_SIDE && p.w <= CROP_MAX_SIDE,
                   "crop_gather_scaled: sample %d: image of %d x %d (sides 1..%d)", i, p.h, p.w, CROP_MAX_SIDE);
    UNETDC_REQUIRE(p.t >= s / 2 && p.t <= 2 * s, "crop_gather_scaled: sample %d: source side %d outside %d..%d", i, p.t, s / 2,
                   2 * s);
    const int ymax = p.h > p.t ? p.h - p.t : 0, xmax = p.w > p.t ? p.w - p.t : 0;
    UNETDC_REQUIRE(p.y0 >= 0 && p.y0 <= ymax && p.x0 >= 0 && p.x0 <= xmax,
                   "crop_gather_scaled: sample %d: origin (%d, %d) outside 0..%d, 0..%d", i, p.y0, p.x0, ymax, xmax);
    const long long hw = (long long)p.h * p.w;
    UNETDC_REQUIRE(p.img_off >= 0 && p.img_off <= images_bytes && hw * c <= images_bytes - p.img_off,
                   "crop_gather_scaled: sample %d: image at offset %lld leaves the buffer of %ld bytes", i, p.img_off,
                   images_bytes);
    UNETDC_REQUIRE(p.mask_off >= 0 && p.mask_off <= masks_bytes && hw <= masks_bytes - p.mask_off,
                   "crop_gather_scaled: sample %d: mask at offset %lld leaves the buffer of %ld bytes", i, p.mask_off,
                   masks_bytes);
    UNETDC_REQUIRE(p.k >= 0 && p.k <= 3, "crop_gather_scaled: sample %d: k = %d (0..3)", i, p.k);
    UNETDC_REQUIRE((p.flags & ~(AUG_HFLIP | AUG_VFLIP | AUG_BC)) == 0, "crop_gather_scaled: sample %d: bad flags 0x%x", i,
                   p.flags);
    UNETDC_REQUIRE(p.field >= -1 && p.field < nfields, "crop_gather_scaled: sample %d: field slot %d outside [-1, %d)", i,
                   p.field, nfields);
    UNETDC_REQUIRE(p.field < 0 || fields, "crop_gather_scaled: sample %d draws elastic but fields is null", i);
  }
  for (int s0 = 0; s0 < n; s0 += AUG_MAX_BATCH) {
    const int m = n - s0 < AUG_MAX_BATCH ? n - s0 : AUG_MAX_BATCH;
    CropScaledBatch b = {};
    for (int i = 0; i < m; ++i) b.r[i] = params[s0 + i];
    hipLaunchKernelGGL(crop_gather_scaled_kernel, dim3(s / 16, s / 16, m), dim3(256), 0, stream, images, masks, c, s, fields, b,
                       s0, out_img, out_mask);
  }
  return n ? check_launch("crop_gather_scaled_kernel") : UNETDC_OK;
}

}  // namespace unetdc
