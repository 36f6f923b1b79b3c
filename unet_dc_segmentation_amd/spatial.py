"""Ripley's K / L of the droplet centroids with simulated patterns on the HIP device (csrc/spatial.hip),
next to the droplet table of ``droplets.py``: it reads the table's sums alone, never the label map.

The yardstick is the host restatement ``utils/spatial_stats.py`` (bit-exact, tests/test_gpu_spatial.py), which also turns the
counts into K, L, the envelope and the test.  Per batch every launch is enqueued on the current stream and the host waits
once: one device->host copy brings each image's points and counts.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

MAX_POINTS = 1 << 20


def spatial_stats_batch(droplet_sums, out_hws, rmax, n_sim, seed, windows=None, masks=None):
    """droplet_sums: (count [B] int32, area [B, cap] int32, sumy [B, cap] int64, sumx [B, cap] int64) device outputs of
    unetdc_ccl_stats / unetdc_split_stats as mask_and_droplets_batch(keep_sums=True) returns them, or None: the 4-connected
    components of `masks` (B [h, w] uint8 device tensors) are then labelled here, as density_maps_batch does.  out_hws: B
    (h, w) pairs; windows: None, or per image None or a [h, w] uint8 device tensor (nonzero = inside).  Returns one dict per
    image: N, n_dropped, A (ints), py, px (int64 [N]) and n, pairs, pairs_all (int64 [(1 + n_sim), rmax + 1])."""
    from utils.spatial_stats import check_radius, check_sims
    R, S = check_radius(rmax), check_sims(n_sim)
    hws = [tuple(int(v) for v in hw) for hw in out_hws]
    B = len(hws)
    if B == 0:
        return []
    windows = [None] * B if windows is None else list(windows)
    if droplet_sums is None and masks is None:
        raise _lib.UnetdcError("spatial_stats_batch without the droplet sums needs the masks to label")
    dev = (droplet_sums[1] if droplet_sums is not None else masks[0]).device
    for win, hw in zip(windows, hws):
        if win is not None and (not win.is_cuda or win.dtype != torch.uint8 or tuple(win.shape) != hw):
            raise _lib.UnetdcError("spatial_stats_batch needs [h, w] uint8 device windows of the images' sizes")
    s = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    caps = [min(int(droplet_sums[1].shape[1]) if droplet_sums is not None else (h * w + 1) // 2, MAX_POINTS) for h, w in hws]
    wsb = max(lib.unetdc_ripley_workspace(h, w, cap, R, S) for (h, w), cap in zip(hws, caps))
    if wsb <= 0:
        raise _lib.UnetdcError("spatial_stats_batch: an image size, radius or simulation count the library refuses")
    if droplet_sums is None:
        wsb = max(wsb, max(lib.unetdc_ccl_workspace(h, w) for h, w in hws))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)                 # one workspace: the launches are stream-ordered
    rows = (1 + S) * (R + 1)
    # one allocation, one copy: the int64 counts of every image (pairs, pairs_all), then its int32 words (info, py, px, n)
    off32 = np.concatenate([[0], np.cumsum([4 + 2 * cap + rows for cap in caps])]).astype(np.int64)
    n64 = 2 * rows * B
    out = torch.empty(8 * n64 + 4 * int(off32[-1]), dtype=torch.uint8, device=dev)
    o64, o32 = out[:8 * n64].view(torch.int64), out[8 * n64:].view(torch.int32)
    keep = []                                                            # ccl outputs: alive until the wait below
    for i, ((h, w), cap, win) in enumerate(zip(hws, caps, windows)):
        if droplet_sums is None:
            mask = masks[i].contiguous()
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            area = torch.empty(cap, dtype=torch.int32, device=dev)
            sy = torch.empty(cap, dtype=torch.int64, device=dev)
            sx = torch.empty(cap, dtype=torch.int64, device=dev)
            _lib.call("unetdc_ccl_stats", mask.data_ptr(), h, w, 1, ws.data_ptr(), ws.numel(), cnt.data_ptr(), area.data_ptr(),
                      sy.data_ptr(), sx.data_ptr(), None, cap, s)
            table = (cnt.data_ptr(), area.data_ptr(), sy.data_ptr(), sx.data_ptr())
            keep.append((cnt, area, sy, sx))
        else:
            cnt, area, sy, sx = droplet_sums
            table = (cnt[i:].data_ptr(), area[i].data_ptr(), sy[i].data_ptr(), sx[i].data_ptr())
        if win is not None:
            win = win.contiguous()
            keep.append(win)
        wptr = None if win is None else win.data_ptr()
        w32 = o32[int(off32[i]):int(off32[i + 1])]
        info, py, px, n = w32[:4], w32[4:4 + cap], w32[4 + cap:4 + 2 * cap], w32[4 + 2 * cap:]
        pairs, pairs_all = o64[2 * rows * i:2 * rows * i + rows], o64[2 * rows * i + rows:2 * rows * (i + 1)]
        _lib.call("unetdc_droplet_points", *table, cap, wptr, h, w, py.data_ptr(), px.data_ptr(), info.data_ptr(), s)
        _lib.call("unetdc_ripley_counts", py.data_ptr(), px.data_ptr(), info.data_ptr(), cap, wptr, h, w, R, S, int(seed) & 0xFFFFFFFF,
                  ws.data_ptr(), ws.numel(), n.data_ptr(), pairs.data_ptr(), pairs_all.data_ptr(), s)
    host = out.cpu().numpy()                                             # the batch's one host wait
    h64, h32 = host[:8 * n64].view(np.int64), host[8 * n64:].view(np.int32)
    res = []
    for i, cap in enumerate(caps):
        w32 = h32[int(off32[i]):int(off32[i + 1])]
        N, dropped, A, flags = (int(v) for v in w32[:4])
        if flags & 1:
            raise _lib.UnetdcError(f"spatial_stats_batch: image {i} has more droplets than the {cap} its table holds")
        counts = h64[2 * rows * i:2 * rows * (i + 1)].reshape(2, 1 + S, R + 1)
        res.append({"N": N, "n_dropped": dropped, "A": A, "py": w32[4:4 + N].astype(np.int64),
                    "px": w32[4 + cap:4 + cap + N].astype(np.int64),
                    "n": w32[4 + 2 * cap:].reshape(1 + S, R + 1).astype(np.int64), "pairs": counts[0].copy(),
                    "pairs_all": counts[1].copy()})
    return res
