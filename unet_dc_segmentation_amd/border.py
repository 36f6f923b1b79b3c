"""The separation weight map of the border-weighted loss (csrc/border.hip), built per batch from the masks
the training loop already holds on the HIP device: ``weight = border_weights(masks, w0)``, then
``utils.metrics_DC.focal_dice_loss(pred, masks, ..., weight=weight)``.

The definition (distances to the nearest and second-nearest 4-connected component inside a (2R + 1)^2 window, the weight from
them) is that of ``utils/border_weights.py``, whose numpy form is the path of CPU tensors and the yardstick of the kernels.
"""
from __future__ import annotations

import torch

from . import _lib


def workspace_bytes(n, h, w, radius):
    """Bytes unetdc_border_weights needs for n images of h x w (0: a geometry it refuses)."""
    return int(_lib.load().unetdc_border_weights_workspace(int(n), int(h), int(w), int(radius)))


def border_weights(target, w0, sigma=5.0, radius=None, out=None, workspace=None, planes=False):
    """target: [..., h, w] masks (foreground where > 0.5; every [h, w] plane is an image of its own) -> fp32 weights of the same
    shape, no gradient: 1 + w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) on background pixels whose second-nearest droplet lies within
    `radius` pixels (default ceil(4 sigma), at most 64), exactly 1 elsewhere.
    out: a contiguous fp32 tensor of the target's shape to write into; workspace: a uint8 tensor of at least
    workspace_bytes(...) on the device (allocated when missing or too small); planes=True: (weights, D1, D2) with the int32
    squared distances.  On the HIP device: five launches on the current stream, nothing waits; CPU tensors take
    utils.border_weights.border_weights_numpy."""
    from utils.border_weights import border_weights_numpy, check_params
    try:
        w0, sigma, radius = check_params(w0, sigma, radius)
    except (ValueError, TypeError) as e:
        raise _lib.UnetdcError(str(e))
    if not torch.is_tensor(target) or target.dim() < 2:
        raise _lib.UnetdcError("border_weights: the target must be a tensor with at least two dimensions")
    shape = tuple(target.shape)
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != target.device):
        raise _lib.UnetdcError(f"border_weights: out must be a contiguous fp32 {list(shape)} tensor on the target's device")
    if not target.is_cuda:
        res = border_weights_numpy(target.detach().float().numpy(), w0, sigma, radius, planes=planes)
        res = tuple(torch.from_numpy(a) for a in res) if planes else (torch.from_numpy(res),)
        if out is not None:
            res = (out.copy_(res[0]),) + res[1:]
        return res if planes else res[0]
    t = target.detach().to(torch.float32).contiguous()
    h, w = shape[-2:]
    n = t.numel() // max(h * w, 1)
    nbytes = workspace_bytes(n, h, w, radius) if h and w else 0
    if nbytes == 0:
        raise _lib.UnetdcError(f"border_weights: {list(shape)} outside the limits (1..65535 images, sides 1..16384, h * w < 2^30)")
    if (workspace is None or workspace.dtype != torch.uint8 or workspace.device != t.device or not workspace.is_contiguous()
            or workspace.numel() < nbytes or workspace.data_ptr() % 4):
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    weight = torch.empty(shape, dtype=torch.float32, device=t.device) if out is None else out
    d1 = torch.empty(shape, dtype=torch.int32, device=t.device) if planes else None
    d2 = torch.empty(shape, dtype=torch.int32, device=t.device) if planes else None
    _lib.call("unetdc_border_weights", t.data_ptr(), n, h, w, w0, sigma, radius, weight.data_ptr(),
              d1.data_ptr() if planes else None, d2.data_ptr() if planes else None, workspace.data_ptr(), workspace.numel(),
              torch.cuda.current_stream().cuda_stream)
    return (weight, d1, d2) if planes else weight
