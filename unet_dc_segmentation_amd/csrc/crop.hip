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

}  // namespace unetdc
