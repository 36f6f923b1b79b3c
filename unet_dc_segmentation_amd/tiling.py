"""Tiled inference at native resolution on the HIP device (csrc/tile.hip): the background-corrected
image is cut into overlapping network-size tiles, the tiles go through the engine, and their probabilities are blended into
one map of the image's size -- the input of ``droplets.mask_and_droplets_batch``, ``evaluate.match_batch`` /
``sweep_batch`` and ``density.density_maps_batch`` at the identity geometry (probability size == output size).

The rules (plan, fold, weights, order of the fp32 operations) are those of ``utils/tiling.py``, whose ``gather_numpy`` /
``blend_numpy`` are the host path of the two kernels.
"""
from __future__ import annotations

import torch

from . import _lib

_plans = {}


def _plan(h, w, T, O, device):
    """(yo, xo) of utils.tiling.tile_plan as device int32 tensors, cached per (h, w, T, O, device); bad limits raise."""
    key = (int(h), int(w), int(T), int(O), str(device))
    if key not in _plans:
        from utils.tiling import tile_plan
        try:
            yo, xo = tile_plan(*key[:4])
        except ValueError as e:
            raise _lib.UnetdcError(str(e))
        _plans[key] = (torch.tensor(yo, dtype=torch.int32, device=device), torch.tensor(xo, dtype=torch.int32, device=device))
    return _plans[key]


def _image(img_u8):
    if not img_u8.is_cuda or img_u8.dtype != torch.uint8 or img_u8.dim() != 3:
        raise _lib.UnetdcError("tiling needs an [H, W, C] uint8 tensor on the HIP device")
    return img_u8.contiguous()


def tile_gather(img_u8, T, O, t0=0, count=None, out=None):
    """img_u8: [H, W, C] uint8 on the HIP device -> the tiles t0 .. t0 + count - 1 of its plan (all from t0 on without count)
    as [count, C, T, T] fp32 in [0, 1] (written into `out` when given); out-of-image pixels are reflected."""
    img_u8 = _image(img_u8)
    h, w, c = img_u8.shape
    yo, xo = _plan(h, w, T, O, img_u8.device)
    count = len(yo) * len(xo) - t0 if count is None else int(count)
    if out is None:
        out = torch.empty(max(count, 0), c, T, T, dtype=torch.float32, device=img_u8.device)
    elif tuple(out.shape) != (count, c, T, T) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != img_u8.device:
        raise _lib.UnetdcError(f"tile_gather: out must be a contiguous fp32 [{count}, {c}, {T}, {T}] tensor on the image's device")
    _lib.call("unetdc_tile_gather_u8_to_chw_f32", img_u8.data_ptr(), h, w, c, out.data_ptr(), int(T), yo.data_ptr(), len(yo),
              xo.data_ptr(), len(xo), int(t0), count, torch.cuda.current_stream().cuda_stream)
    return out


def tile_blend(tile_probs, h, w, T, O):
    """tile_probs: [n_tiles, T, T] fp32 on the HIP device, the probabilities of the tiles of the plan of (h, w, T, O) in tile
    order -> [h, w] fp32: the weighted mean of the tiles that cover each pixel (one launch, no atomics)."""
    if not tile_probs.is_cuda or tile_probs.dtype != torch.float32 or tile_probs.dim() != 3:
        raise _lib.UnetdcError("tile_blend needs an [n_tiles, T, T] fp32 tensor on the HIP device")
    yo, xo = _plan(h, w, T, O, tile_probs.device)
    if tuple(tile_probs.shape) != (len(yo) * len(xo), T, T):
        raise _lib.UnetdcError(f"tile_blend: {tuple(tile_probs.shape)} tiles, the plan of {h} x {w} has {(len(yo) * len(xo), T, T)}")
    tile_probs = tile_probs.contiguous()
    out = torch.empty(int(h), int(w), dtype=torch.float32, device=tile_probs.device)
    _lib.call("unetdc_tile_blend_f32", tile_probs.data_ptr(), int(T), int(O), yo.data_ptr(), len(yo), xo.data_ptr(), len(xo),
              out.data_ptr(), int(h), int(w), torch.cuda.current_stream().cuda_stream)
    return out


@torch.no_grad()
def predict_tiled(model, img_u8, T, O, batch, tta=1, envelope=False):
    """img_u8: [H, W, C] uint8 on the HIP device (background-corrected) -> [H, W] fp32 probabilities on the device.
    The tiles are gathered and forwarded `batch` at a time (a ragged last chunk is a second engine shape), every chunk's output
    is copied into its slice of one [n_tiles, T, T] buffer, and ONE blend launch makes the map.  Nothing waits for the device.
    tta > 1: the tiles go in groups of max(1, batch // tta), and a group's slice of the buffer is the mean
    over the `tta` flipped and rotated variants of its tiles (tta.group_mean, `batch` items per forward).
    envelope: -> (mean, lo, hi), three [H, W] maps: every group's one launch also leaves the per-tile minimum and maximum over the
    variants (tta.dihedral_mean_env), and lo and hi go through the same blend -- they are the blend of the per-tile envelopes,
    not the envelope of blended maps."""
    img_u8 = _image(img_u8)
    h, w, _ = img_u8.shape
    yo, xo = _plan(h, w, T, O, img_u8.device)
    n, batch = len(yo) * len(xo), max(1, int(batch))
    probs = torch.empty(3 if envelope else 1, n, T, T, dtype=torch.float32, device=img_u8.device)
    if envelope:
        from utils.tta import check_tta, groups
        from .tta import group_mean
        try:
            tta = check_tta(tta)
        except (ValueError, TypeError) as e:
            raise _lib.UnetdcError(f"predict_tiled: {e}")
        for t0, cnt in groups(n, tta, batch):
            group_mean(model, tile_gather(img_u8, T, O, t0, cnt), tta, batch, tuple(p[t0:t0 + cnt] for p in probs), True)
        return tuple(tile_blend(p, h, w, T, O) for p in probs)
    probs = probs[0]
    if tta != 1:
        from utils.tta import check_tta, groups
        from .tta import group_mean
        try:
            tta = check_tta(tta)
        except (ValueError, TypeError) as e:
            raise _lib.UnetdcError(f"predict_tiled: {e}")
        for t0, cnt in groups(n, tta, batch):
            group_mean(model, tile_gather(img_u8, T, O, t0, cnt), tta, batch, probs[t0:t0 + cnt])
    else:
        for t0 in range(0, n, batch):
            cnt = min(batch, n - t0)
            probs[t0:t0 + cnt].copy_(model(tile_gather(img_u8, T, O, t0, cnt))[:, 0])
    return tile_blend(probs, h, w, T, O)
