"""Training augmentation on the HIP device (csrc/augment.hip): the random part of ``utils.data_loader.TrainAugment`` -- flips,
90-degree rotations, brightness / contrast, elastic deformation -- applied per batch to images already on the device.

Parameters are drawn on the host (:func:`draw_params`, one generator per ``(seed, epoch, index)``) and reach the kernels BY VALUE
in the launch arguments: no device memory is written by the host per batch, so nothing here waits on the device.  The numpy
restatement the kernels are checked against is ``tests/augment_ref.py``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

HFLIP, VFLIP, BC = 1, 2, 4          # include/unetdc_hip.h UNETDC_AUG_*
ELASTIC_ALPHA, ELASTIC_SIGMA = 1.0, 50.0        # TrainAugment's _elastic(alpha=1, sigma=50)

# unetdc_augment_params: int32 src, flags, k, field; float32 alpha, beta_max; int32 reserved[2]
PARAMS_DTYPE = np.dtype([("src", "<i4"), ("flags", "<i4"), ("k", "<i4"), ("field", "<i4"), ("alpha", "<f4"),
                         ("beta_max", "<f4"), ("reserved", "<i4", (2,))])


def draw_params(seed, epoch, index):
    """TrainAugment's draws for one sample, from np.random.default_rng([seed, epoch, index]): the same probabilities and
    ranges in the same order (hflip .5, vflip .2, rot90 .5 with k in {1, 2, 3}, brightness / contrast .2, elastic .3), the
    elastic noise replaced by a 32-bit field seed.  Independent of batch composition, world size and worker count."""
    rng = np.random.default_rng([int(seed), int(epoch), int(index)])
    p = dict(hflip=bool(rng.random() < 0.5), vflip=bool(rng.random() < 0.2), k=0, bc=False, alpha=1.0, beta=0.0,
             elastic=False, field_seed=0)
    if rng.random() < 0.5:
        p["k"] = int(rng.integers(1, 4))
    if rng.random() < 0.2:
        p["bc"], p["alpha"], p["beta"] = True, 1.0 + rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)
    if rng.random() < 0.3:
        p["elastic"], p["field_seed"] = True, int(rng.integers(0, 2 ** 32))
    return p


def pack_draws(rec, params, img_max):
    """Fill flags, k, alpha, beta_max and field of the records `rec` (PARAMS_DTYPE or one of crops' record types) from the
    draw_params dicts and per-image maxima -> field seeds: the samples that draw elastic get field slots 0, 1, ... in batch
    order."""
    seeds = []
    for r, p, mx in zip(rec, params, img_max):
        r["flags"] = (HFLIP if p["hflip"] else 0) | (VFLIP if p["vflip"] else 0) | (BC if p["bc"] else 0)
        r["k"] = p["k"]
        r["alpha"] = np.float32(p["alpha"])
        r["beta_max"] = np.float32(p["beta"] * float(mx))                 # formed in double, like beta * float(img.max())
        r["field"] = len(seeds) if p["elastic"] else -1
        if p["elastic"]:
            seeds.append(p["field_seed"])
    return np.asarray(seeds, dtype=np.uint32)


def pack_params(params, src, img_max):
    """[dict from draw_params] + cache indices + per-image maxima -> (unetdc_augment_params records, field seeds)."""
    rec = np.zeros(len(params), dtype=PARAMS_DTYPE)
    rec["src"] = np.asarray(src, dtype=np.int32).reshape(len(params))
    return rec, pack_draws(rec, params, img_max)


def fields_workspace_bytes(n, h, w, sigma=ELASTIC_SIGMA):
    nbytes = _lib.load().unetdc_elastic_fields_workspace(n, h, w, float(sigma))
    if nbytes < 0:
        raise _lib.UnetdcError(f"elastic fields: unsupported geometry n={n} h={h} w={w} sigma={sigma}")
    return nbytes


def elastic_fields(seeds, h, w, sigma=ELASTIC_SIGMA, alpha=ELASTIC_ALPHA, out=None, workspace=None, device="cuda"):
    """uint32 seeds [n] (host) -> displacement fields [n, 2, h, w] float32 on the device ([:, 0] = dx, [:, 1] = dy)."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    n = len(seeds)
    if out is None:
        out = torch.empty(n, 2, h, w, dtype=torch.float32, device=device)
    nbytes = fields_workspace_bytes(n, h, w, sigma)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
    if out.numel() < n * 2 * h * w or workspace.numel() < nbytes:
        raise _lib.UnetdcError("elastic_fields: output or workspace too small")
    _lib.call("unetdc_elastic_fields", seeds.ctypes.data, n, h, w, float(sigma), float(alpha), out.data_ptr(),
              workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(out.device).cuda_stream)
    return out


def augment_gather(cache_img, cache_mask, rec, fields=None, out_img=None, out_mask=None):
    """cache_img [M, C, H, W] float32, cache_mask [M, H, W] uint8 (device), rec: PARAMS_DTYPE records (host) ->
    (images [N, C, H, W], masks [N, 1, H, W]) float32 on the device."""
    if not (cache_img.is_cuda and cache_img.dtype == torch.float32 and cache_img.dim() == 4 and cache_img.is_contiguous()):
        raise _lib.UnetdcError("augment_gather: cache_img must be a contiguous [M, C, H, W] float32 tensor on the HIP device")
    m, c, h, w = cache_img.shape
    if cache_mask.dtype != torch.uint8 or tuple(cache_mask.shape) != (m, h, w) or not cache_mask.is_contiguous():
        raise _lib.UnetdcError("augment_gather: cache_mask must be a contiguous [M, H, W] uint8 tensor")
    rec = np.ascontiguousarray(rec, dtype=PARAMS_DTYPE)
    n = len(rec)
    dev = cache_img.device
    if out_img is None:
        out_img = torch.empty(n, c, h, w, dtype=torch.float32, device=dev)
    if out_mask is None:
        out_mask = torch.empty(n, 1, h, w, dtype=torch.float32, device=dev)
    if tuple(out_img.shape) != (n, c, h, w) or tuple(out_mask.shape) != (n, 1, h, w):
        raise _lib.UnetdcError("augment_gather: output shapes do not match the batch")
    nfields = 0
    if fields is not None:
        if tuple(fields.shape[1:]) != (2, h, w) or fields.dtype != torch.float32:
            raise _lib.UnetdcError("augment_gather: fields must be [n, 2, H, W] float32")
        nfields = fields.shape[0]
    _lib.call("unetdc_augment_gather", cache_img.data_ptr(), cache_mask.data_ptr(), m, c, h, w, rec.ctypes.data, n,
              fields.data_ptr() if fields is not None else None, nfields, out_img.data_ptr(), out_mask.data_ptr(),
              torch.cuda.current_stream(dev).cuda_stream)
    return out_img, out_mask
