"""Deep (16-bit) images on the HIP device (csrc/window.hip): order statistics by radix select, the integer
window to 8 bits, the maximum over the planes of a stack.  utils/intensity_window.py is the derivation of the rules and the
yardstick (bit-exact, tests/test_gpu_intensity.py).

A 16-bit image lives on the device as a tensor of 16-bit words, dtype torch.uint16 or torch.int16: only the bits are read.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

# csrc/window.hip (tests/test_intensity_cpu.py holds the two files together)
WIN_THREADS = 256
WIN_HIST_MAX_GROUPS = 256
WIN_MAX_GROUPS = 1024
WIN_MAX_RANKS = 8
WIN_MAX_PLANES = 256
HIST_PIXELS_PER_TRIP = WIN_HIST_MAX_GROUPS * WIN_THREADS * 8       # win_hist_kernel: 8 pixels per thread and trip


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _words(t, dims, who):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.uint16, torch.int16) and t.dim() == dims):
        raise _lib.UnetdcError(f"{who} needs a {dims}-dimensional 16-bit tensor (torch.uint16 or torch.int16) on the HIP device")
    return t.contiguous()


def upload_u16(arr_u16_host, device="cuda"):
    """numpy uint16 -> device tensor of the same words (dtype int16: the one 16-bit dtype every torch copy takes)."""
    a = np.ascontiguousarray(arr_u16_host)
    if a.dtype != np.uint16:
        raise _lib.UnetdcError("upload_u16 needs a uint16 array")
    return torch.from_numpy(a.view(np.int16)).to(device)


def ranks_device(t_u16, ppm):
    """[h, w, c] 16-bit device tensor, ppm: 1..8 integers in 0..10^6 -> (value, below, equal), int32 [c, nq] device tensors.
    Nothing comes back to the host."""
    t = _words(t_u16, 3, "ranks_device")
    h, w, c = t.shape
    req = np.asarray([int(p) for p in ppm], np.int32)
    nq = len(req)
    nbytes = _lib.load().unetdc_u16_ranks_workspace(h, w, c, nq)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=t.device)
    out = torch.empty(3, max(c, 1), max(nq, 1), dtype=torch.int32, device=t.device)
    _lib.call("unetdc_u16_ranks", t.data_ptr(), h, w, c, req.ctypes.data, nq, ws.data_ptr(), nbytes, out[0].data_ptr(),
              out[1].data_ptr(), out[2].data_ptr(), _stream())
    return out[0], out[1], out[2]


def window_device(t_u16, levels, dc=None):
    """[h, w, c] 16-bit device tensor, levels: int32 [c, 2] DEVICE tensor -> uint8 [h, w, dc] (dc = c, or 3 with c = 1)."""
    t = _words(t_u16, 3, "window_device")
    h, w, c = t.shape
    dc = c if dc is None else int(dc)
    if not (torch.is_tensor(levels) and levels.is_cuda and levels.dtype == torch.int32 and levels.numel() == 2 * c):
        raise _lib.UnetdcError("window_device needs the levels as an int32 [c, 2] tensor on the HIP device")
    levels = levels.contiguous()
    out = torch.empty(h, w, dc, dtype=torch.uint8, device=t.device)
    _lib.call("unetdc_window_u16_to_u8", t.data_ptr(), h, w, c, levels.data_ptr(), out.data_ptr(), dc, _stream())
    return out


def planes_max_device(t):
    """[P, h, w] 16-bit device tensor -> [h, w]: the maximum over the planes."""
    t = _words(t, 3, "planes_max_device")
    p, h, w = t.shape
    out = torch.empty(h, w, dtype=t.dtype, device=t.device)
    _lib.call("unetdc_planes_max_u16", t.data_ptr(), p, h, w, out.data_ptr(), _stream())
    return out


_fixed = {}


def _fixed_levels(spec, c, device):
    """The run's fixed levels as a device tensor, uploaded once per (levels, channels, device)."""
    key = (spec.levels, c, str(device))
    if key not in _fixed:
        _fixed[key] = torch.tensor([list(spec.levels)] * c, dtype=torch.int32).to(device)
    return _fixed[key]


def deep_to_u8_device(arr_u16_host, spec, device="cuda"):
    """The stage on the device: numpy uint16 [h, w, c] (utils.intensity_window.decode_deep) and a WindowSpec -> (uint8 device
    tensor [h, w, 3 or c], record).  record: {"ranks": int32 [3, c, 5], "levels": int32 [c, 2]} as DEVICE tensors -- one ranks call
    for the five requests of spec.ppm; the percentile levels go from its output to the window without leaving the device.
    record_host() fetches a record for utils.intensity_window.record_row."""
    from utils.intensity_window import out_channels
    t = upload_u16(arr_u16_host, device)
    c = t.shape[2]
    value, below, equal = ranks_device(t, spec.ppm)
    if spec.levels is None:
        levels = torch.stack((value[:, 1], value[:, 3]), dim=1).contiguous()
    else:
        levels = _fixed_levels(spec, c, t.device)
    return window_device(t, levels, out_channels(c)), {"ranks": torch.stack((value, below, equal)), "levels": levels}


def record_host(record):
    """A record of deep_to_u8_device -> numpy arrays (the stage's only copy from the device)."""
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in record.items()}
