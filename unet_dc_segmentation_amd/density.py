"""Radial and spatial droplet density maps on the HIP device (csrc/density.hip): the ROI, ring and Gaussian-density analysis of
the reference's ``quantify_pipline.py`` at the original image size, next to the droplet table of ``droplets.py``.

The yardstick is the host restatement ``utils/density.py`` (bit-exact, tests/test_gpu_density.py).  Per batch every launch is
enqueued on the current stream and the host waits once: one device->host copy brings each image's numbers
(``unetdc_density_stats``) and its two uint8 colormap index planes.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

# mirrors unetdc_density_stats (include/unetdc_hip.h; abi.hip asserts its size and offsets)
STATS_DTYPE = np.dtype([("roi_area", "<i8"), ("m10", "<i8"), ("m01", "<i8"), ("cx", "<i4"), ("cy", "<i4"),
                        ("otsu_threshold", "<i4"), ("nb_layers", "<i4"), ("max_ring_distance", "<f8"), ("ndroplets", "<i4"),
                        ("radial_min_bits", "<u4"), ("radial_max_bits", "<u4"), ("spatial_min_bits", "<u4"),
                        ("spatial_max_bits", "<u4"), ("ring_count", "<i4", (255,))])
assert STATS_DTYPE.itemsize == 1088
MIN_SIDE = 2
MAX_LAYERS = 255


def density_maps_batch(rgb_dev_list, masks, droplet_sums, nb_layers=10, kernel_size=21, planes=False):
    """rgb_dev_list: B decoded [h, w, 3] uint8 images on the HIP device (before the rolling ball); masks: B [h, w] uint8 {0, 1}
    device tensors of the same sizes.  droplet_sums: (count [B] int32, area [B, cap] int32, sumy [B, cap] int64, sumx [B, cap]
    int64) device outputs of unetdc_ccl_stats made with min_area = 1 and holding every droplet, or None: the components are
    then labelled here.  Returns one dict per image: threshold, roi_area, cx, cy, max_ring_distance, ring_counts (int64
    [nb_layers]), radial_index and spatial_index (uint8 [h, w], host), and with planes=True the device planes blur, roi,
    ring, radial and spatial."""
    from utils.density import gaussian_taps
    B = len(rgb_dev_list)
    if B == 0:
        return []
    dev = masks[0].device
    s = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    hws = [tuple(int(v) for v in m.shape) for m in masks]
    for rgb, (h, w) in zip(rgb_dev_list, hws):
        if not rgb.is_cuda or rgb.dtype != torch.uint8 or tuple(rgb.shape) != (h, w, 3):
            raise _lib.UnetdcError("density_maps_batch needs [h, w, 3] uint8 device images matching the masks")
    sigma = kernel_size / 6
    taps = gaussian_taps(sigma)
    wsb = max(lib.unetdc_density_workspace(h, w) for h, w in hws)
    if droplet_sums is None:
        wsb = max(wsb, max(lib.unetdc_ccl_workspace(h, w) for h, w in hws))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)        # one workspace: the launches are stream-ordered
    sizes = [h * w for h, w in hws]
    offs = np.concatenate([[0], np.cumsum([2 * n for n in sizes])]).astype(np.int64) + B * STATS_DTYPE.itemsize
    out = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)     # stats of every image, then its two index planes
    keep = []                                                            # ccl outputs: alive until the wait below
    plane_of = {}                                                        # image -> its optional intermediate planes
    for i, ((h, w), rgb, mask) in enumerate(zip(hws, rgb_dev_list, masks)):
        rgb, mask = rgb.contiguous(), mask.contiguous()
        if droplet_sums is None:
            cap = (h * w + 1) // 2                                       # the most 4-connected components h x w can hold
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            area = torch.empty(cap, dtype=torch.int32, device=dev)
            sy = torch.empty(cap, dtype=torch.int64, device=dev)
            sx = torch.empty(cap, dtype=torch.int64, device=dev)
            _lib.call("unetdc_ccl_stats", mask.data_ptr(), h, w, 1, ws.data_ptr(), ws.numel(), cnt.data_ptr(),
                      area.data_ptr(), sy.data_ptr(), sx.data_ptr(), None, cap, s)
            dptr = (cnt.data_ptr(), area.data_ptr(), sy.data_ptr(), sx.data_ptr(), cap)
            keep.append((cnt, area, sy, sx))
        else:
            cnt, area, sy, sx = droplet_sums
            dptr = (cnt[i:].data_ptr(), area[i].data_ptr(), sy[i].data_ptr(), sx[i].data_ptr(), int(area.shape[1]))
        st = out[i * STATS_DTYPE.itemsize:]
        ri = out[int(offs[i]):int(offs[i]) + h * w]
        si = out[int(offs[i]) + h * w:int(offs[i + 1])]
        pp = [None] * 5
        if planes:
            u8 = lambda: torch.empty(h, w, dtype=torch.uint8, device=dev)
            f32 = lambda: torch.empty(h, w, dtype=torch.float32, device=dev)
            plane_of[i] = {"blur": u8(), "roi": u8(), "ring": u8(), "radial": f32(), "spatial": f32()}
            pp = [plane_of[i][k].data_ptr() for k in ("blur", "roi", "ring", "radial", "spatial")]
        _lib.call("unetdc_density_maps", rgb.data_ptr(), mask.data_ptr(), h, w, *dptr, int(nb_layers), float(sigma),
                  taps.ctypes.data, ws.data_ptr(), ws.numel(), st.data_ptr(), ri.data_ptr(), si.data_ptr(), *pp, s)
    host = out.cpu().numpy()                                             # the batch's one host wait
    stats = host[:B * STATS_DTYPE.itemsize].view(STATS_DTYPE)
    res = []
    for i, (h, w) in enumerate(hws):
        st = stats[i]
        r = {"threshold": int(st["otsu_threshold"]), "roi_area": int(st["roi_area"]), "cx": int(st["cx"]),
             "cy": int(st["cy"]), "max_ring_distance": float(st["max_ring_distance"]),
             "ring_counts": st["ring_count"][:nb_layers].astype(np.int64), "ndroplets": int(st["ndroplets"]),
             "radial_index": host[int(offs[i]):int(offs[i]) + h * w].reshape(h, w),
             "spatial_index": host[int(offs[i]) + h * w:int(offs[i + 1])].reshape(h, w)}
        r.update(plane_of.get(i, {}))
        res.append(r)
    return res


def density_sqrt(x):
    """sqrt of an int64 device tensor with the square root the density kernels use (fp64 device tensor)."""
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    _lib.call("unetdc_density_sqrt", x.data_ptr(), out.data_ptr(), x.numel(), torch.cuda.current_stream().cuda_stream)
    return out
