"""Test-time augmentation on the HIP device (csrc/tta.hip): the flipped and rotated variants of a batch go
through the engine, and the mean of their outputs, each mapped back first, is the probability map every consumer behind the
forward reads (``droplets.mask_and_droplets_batch``, ``evaluate.match_batch`` / ``sweep_batch``, ``density.density_maps_batch``).

The rule (variants, their order, the order of the fp32 operations, the chunk rule) is that of ``utils/tta.py``, whose
``expand_numpy`` / ``mean_numpy`` are the host path of the two kernels.
"""
from __future__ import annotations

import torch

from . import _lib


def _check(t, ndim, N, what):
    from utils.tta import MAX_CHANNELS, MAX_IMAGES, MAX_SIDE, MIN_SIDE, check_tta
    try:
        N = check_tta(N)
    except (ValueError, TypeError) as e:
        raise _lib.UnetdcError(f"{what}: {e}")
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != ndim:
        raise _lib.UnetdcError(f"{what} needs a {ndim}-dimensional fp32 tensor on the HIP device")
    s = t.shape[-1]
    if t.shape[-2] != s or s % 16 or not MIN_SIDE <= s <= MAX_SIDE:
        raise _lib.UnetdcError(f"{what}: square planes with a side that is a multiple of 16 in {MIN_SIDE}..{MAX_SIDE}, not "
                               f"{tuple(t.shape)}")
    if not 1 <= t.shape[0] <= MAX_IMAGES * (N if ndim == 3 else 1) or (ndim == 4 and not 1 <= t.shape[1] <= MAX_CHANNELS):
        raise _lib.UnetdcError(f"{what}: {tuple(t.shape)} outside the limits (1..{MAX_IMAGES} images, 1..{MAX_CHANNELS} channels)")
    return t.contiguous(), N


def _out(out, shape, like, what):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if (not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous()
            or out.device != like.device):
        raise _lib.UnetdcError(f"{what}: out must be a contiguous fp32 {list(shape)} tensor on the input's device")
    return out


def dihedral_expand(x, N, out=None):
    """x: [n, C, S, S] fp32 on the HIP device -> [n * N, C, S, S]: item b * N + i is variant utils.tta.variants(N)[i] of image b
    (written into `out` when given; a permutation, bit-exact)."""
    x, N = _check(x, 4, N, "dihedral_expand")
    n, c, s, _ = x.shape
    out = _out(out, (n * N, c, s, s), x, "dihedral_expand")
    _lib.call("unetdc_dihedral_expand_f32", x.data_ptr(), n, c, s, N, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def dihedral_mean(p, N, out=None):
    """p: [n * N, S, S] fp32 on the HIP device, item b * N + i the output on variant i of image b -> [n, S, S]: the items mapped
    back and averaged in list order (written into `out` when given; utils.tta.mean_numpy bit for bit)."""
    p, N = _check(p, 3, N, "dihedral_mean")
    if p.shape[0] % N:
        raise _lib.UnetdcError(f"dihedral_mean: {p.shape[0]} items are no multiple of {N} variants")
    n, s = p.shape[0] // N, p.shape[-1]
    out = _out(out, (n, s, s), p, "dihedral_mean")
    _lib.call("unetdc_dihedral_mean_f32", p.data_ptr(), n, s, N, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def dihedral_mean_env(p, N, out=None):
    """p as for dihedral_mean -> (mean, lo, hi), [n, S, S] each, from ONE pass over the items: the mean of dihedral_mean bit for
    bit, and the per-pixel minimum and maximum over the mapped-back items (utils.tta.mean_env_numpy).  out: the three tensors to
    write into.  Only lo <= hi holds; the rounded mean may lie outside them."""
    p, N = _check(p, 3, N, "dihedral_mean_env")
    if p.shape[0] % N:
        raise _lib.UnetdcError(f"dihedral_mean_env: {p.shape[0]} items are no multiple of {N} variants")
    n, s = p.shape[0] // N, p.shape[-1]
    if out is not None and len(out) != 3:
        raise _lib.UnetdcError("dihedral_mean_env: out is the three tensors (mean, lo, hi)")
    outs = tuple(_out(None if out is None else o, (n, s, s), p, "dihedral_mean_env") for o in (out or (None,) * 3))
    _lib.call("unetdc_dihedral_mean_env_f32", p.data_ptr(), n, s, N, *(o.data_ptr() for o in outs),
              torch.cuda.current_stream().cuda_stream)
    return outs


def group_mean(model, x, N, batch, out, envelope=False):
    """One group of the chunk rule: x [g, C, S, S] is expanded once, its g * N items go through `model` in slices of `batch` into
    one buffer, and one mean writes out [g, S, S].  envelope: out is the three tensors (mean, lo, hi) and the one launch is
    dihedral_mean_env."""
    items = dihedral_expand(x, N)
    p = torch.empty(items.shape[0], items.shape[2], items.shape[3], dtype=torch.float32, device=x.device)
    for i in range(0, len(items), batch):
        p[i:i + batch].copy_(model(items[i:i + batch])[:, 0])
    return dihedral_mean_env(p, N, out=out) if envelope else dihedral_mean(p, N, out=out)


@torch.no_grad()
def predict_tta(model, x, N, batch, envelope=False):
    """x: [n, C, S, S] fp32 on the HIP device -> [n, 1, S, S] fp32 probabilities on the device: the mean of `model` over the N
    variants of every image.  The images go in groups of max(1, batch // N) (utils.tta.groups: at most two engine shapes);
    nothing waits for the device.  envelope: -> (mean, lo, hi), three tensors of that shape (dihedral_mean_env)."""
    from utils.tta import groups
    x, N = _check(x, 4, N, "predict_tta")
    batch = max(1, int(batch))
    out = torch.empty(3 if envelope else 1, x.shape[0], 1, x.shape[2], x.shape[3], dtype=torch.float32, device=x.device)
    for b0, g in groups(x.shape[0], N, batch):
        if envelope:
            group_mean(model, x[b0:b0 + g], N, batch, tuple(o[b0:b0 + g, 0] for o in out), True)
        else:
            group_mean(model, x[b0:b0 + g], N, batch, out[0, b0:b0 + g, 0])
    return tuple(out) if envelope else out[0]
