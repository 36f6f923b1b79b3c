"""Random crops at native resolution on the HIP device (csrc/crop.hip): S x S windows of images cached
at their own size as HWC uint8, cut, scaled to [0, 1] and augmented by one kernel per batch.  The rule and its numpy path are
``utils/crops.py``; the records reach the kernel BY VALUE in the launch arguments, so nothing here waits on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .augment import pack_draws

# unetdc_crop_params: int64 img_off, mask_off; int32 h, w, y0, x0, flags, k, field; float32 alpha, beta_max; int32 reserved
CROP_DTYPE = np.dtype([("img_off", "<i8"), ("mask_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("y0", "<i4"), ("x0", "<i4"),
                       ("flags", "<i4"), ("k", "<i4"), ("field", "<i4"), ("alpha", "<f4"), ("beta_max", "<f4"),
                       ("reserved", "<i4")])
assert CROP_DTYPE.itemsize == 56
# unetdc_crop_scaled_params: the same record with the side t of the source window where unetdc_crop_params has `reserved`
CROP_SCALED_DTYPE = np.dtype([(n, CROP_DTYPE.fields[n][0]) for n in CROP_DTYPE.names[:-1]] + [("t", "<i4")])
assert CROP_SCALED_DTYPE.itemsize == 56 and CROP_SCALED_DTYPE.fields["t"][1] == CROP_DTYPE.fields["reserved"][1]

IDENTITY = dict(hflip=False, vflip=False, k=0, bc=False, alpha=1.0, beta=0.0, elastic=False, field_seed=0)


def pack_crops(params, img_off, mask_off, sizes, origins, img_max):
    """[augment.draw_params dicts] + per-sample byte offsets, (h, w), (y0, x0) and whole-image maxima -> (unetdc_crop_params
    records, field seeds): the samples that draw elastic get field slots 0, 1, ... in batch order."""
    return _pack(CROP_DTYPE, params, img_off, mask_off, sizes, origins, img_max)


def pack_crops_scaled(params, img_off, mask_off, sizes, origins, img_max, ts):
    """pack_crops for unetdc_crop_gather_scaled: `origins` are those of the source windows, `ts` their sides ->
    (unetdc_crop_scaled_params records, field seeds)."""
    rec, seeds = _pack(CROP_SCALED_DTYPE, params, img_off, mask_off, sizes, origins, img_max)
    rec["t"] = np.asarray(ts, dtype=np.int32).reshape(len(params))
    return rec, seeds


def _pack(dtype, params, img_off, mask_off, sizes, origins, img_max):
    rec = np.zeros(len(params), dtype=dtype)
    for r, io, mo, (h, w), (y0, x0) in zip(rec, img_off, mask_off, sizes, origins):
        r["img_off"], r["mask_off"], r["h"], r["w"], r["y0"], r["x0"] = io, mo, h, w, y0, x0
    return rec, pack_draws(rec, params, img_max)


def crop_gather(images_u8, masks_u8, channels, S, rec, fields=None, out_img=None, out_mask=None):
    """images_u8 / masks_u8: flat uint8 device tensors holding every cached image (HWC) / mask back to back; rec: CROP_DTYPE
    records (host) -> (images [N, C, S, S], masks [N, 1, S, S]) float32 on the device."""
    return _gather("unetdc_crop_gather", CROP_DTYPE, images_u8, masks_u8, channels, S, rec, fields, out_img, out_mask)


def crop_gather_scaled(images_u8, masks_u8, channels, S, rec, fields=None, out_img=None, out_mask=None):
    """crop_gather with CROP_SCALED_DTYPE records: every sample's rec["t"] x rec["t"] source window is resampled to S x S in
    the same kernel pass (unetdc_crop_gather_scaled; the rule: utils.crops.window_scaled)."""
    return _gather("unetdc_crop_gather_scaled", CROP_SCALED_DTYPE, images_u8, masks_u8, channels, S, rec, fields, out_img,
                   out_mask)


def _gather(symbol, dtype, images_u8, masks_u8, channels, S, rec, fields, out_img, out_mask):
    for t, what in ((images_u8, "images_u8"), (masks_u8, "masks_u8")):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous()):
            raise _lib.UnetdcError(f"crop_gather: {what} must be a flat contiguous uint8 tensor on the HIP device")
    if getattr(rec, "dtype", dtype) != dtype:               # (a cast between the two record types would go by position)
        raise _lib.UnetdcError(f"{symbol}: records of another type (its own has {', '.join(dtype.names)})")
    rec = np.ascontiguousarray(rec, dtype=dtype)
    n, c, S = len(rec), int(channels), int(S)
    dev = images_u8.device
    if out_img is None:
        out_img = torch.empty(n, c, S, S, dtype=torch.float32, device=dev)
    if out_mask is None:
        out_mask = torch.empty(n, 1, S, S, dtype=torch.float32, device=dev)
    if tuple(out_img.shape) != (n, c, S, S) or tuple(out_mask.shape) != (n, 1, S, S) or out_img.dtype != torch.float32 or \
            out_mask.dtype != torch.float32 or not (out_img.is_contiguous() and out_mask.is_contiguous()):
        raise _lib.UnetdcError("crop_gather: outputs must be contiguous float32 [N, C, S, S] and [N, 1, S, S]")
    nfields = 0
    if fields is not None:
        if tuple(fields.shape[1:]) != (2, S, S) or fields.dtype != torch.float32 or not fields.is_contiguous():
            raise _lib.UnetdcError("crop_gather: fields must be [n, 2, S, S] float32")
        nfields = fields.shape[0]
    _lib.call(symbol, images_u8.data_ptr(), images_u8.numel(), masks_u8.data_ptr(), masks_u8.numel(), c, S,
              rec.ctypes.data, n, fields.data_ptr() if fields is not None else None, nfields, out_img.data_ptr(),
              out_mask.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out_img, out_mask
