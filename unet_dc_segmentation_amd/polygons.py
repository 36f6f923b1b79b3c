"""Polygon annotations into label maps on the HIP device (csrc/polyfill.hip): the inverse of
``outlines.py``, beside it and ``evaluate.py``.

The yardstick is the host restatement ``utils.polygon_masks.rasterize_numpy`` (bit-exact, tests/test_gpu_polygons.py), whose
``pack`` also makes the arrays read here.  The device fills with each polygon's *rank* among the image's distinct labels (1..U,
ascending: the largest rank is the largest label), so the census is a dense table however large the labels are; one lookup
then writes the labels themselves or, with compact, the dense numbers of the labels that own a pixel.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def rasterize_batch(packed_list, hws, compact=True, device="cuda"):
    """packed_list: per image the record of utils.polygon_masks.pack; hws: per image (h, w).  One upload of all packed arrays;
    per image unetdc_polygon_fill and unetdc_label_census are enqueued back to back on the current stream into ONE workspace;
    the host waits ONCE, on the copy of the census, and then enqueues the unetdc_label_relabel launches.
    -> per image {"labels": int32 DEVICE [h, w], "kept": int64 [K], "area": int64 [K]}: the record of rasterize_numpy."""
    B = len(packed_list)
    if len(hws) != B:
        raise _lib.UnetdcError("rasterize_batch needs one (h, w) per packed record")
    if B == 0:
        return []
    lib = _lib.load()
    dev = torch.device(device)
    hws = [(int(h), int(w)) for h, w in hws]
    uniq, parts, geo = [], [[], [], [], []], []
    for pk in packed_list:
        lab = np.asarray(pk["poly_label"], dtype=np.int64)
        if len(lab) and lab.min() < 1:
            raise _lib.UnetdcError("rasterize_batch: labels are positive")
        u = np.unique(lab)
        uniq.append(u)
        arrays = (np.ascontiguousarray(pk["verts"], dtype=np.int32).reshape(-1), np.asarray(pk["ring_first"], dtype=np.int32),
                  np.asarray(pk["poly_first_ring"], dtype=np.int32), (np.searchsorted(u, lab) + 1).astype(np.int32))
        for dst, a in zip(parts, arrays):
            dst.append(a)
        geo.append((len(lab), len(arrays[1]) - 1, len(arrays[0]) // 2))
    sizes = [lib.unetdc_polygon_fill_workspace(h, w, *g) for (h, w), g in zip(hws, geo)]
    if min(sizes) < 0:
        raise _lib.UnetdcError("rasterize_batch: a geometry the library refuses (sides 1..16384, h * w < 2^30, polygons <= 2^22, "
                               "vertices <= 2^24, polygons * h < 2^31)")
    # the vertex pairs first: every one then starts at an even int32 of the upload, as the kernels' 8-byte loads need
    flat = [a for group in parts for a in group]
    at = np.concatenate([[0], np.cumsum([len(a) for a in flat])]).astype(np.int64)
    up = torch.from_numpy(np.concatenate(flat)).to(dev) if at[-1] else torch.zeros(1, dtype=torch.int32, device=dev)
    ptr = lambda kind, i: up.data_ptr() + 4 * int(at[kind * B + i])
    ws = torch.empty(max(max(sizes), 1), dtype=torch.uint8, device=dev)             # one workspace: the launches are stream-ordered
    first = np.concatenate([[0], np.cumsum([len(u) for u in uniq])]).astype(np.int64)
    area_d = torch.empty(max(int(first[-1]), 1), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    labels = []
    for i, ((h, w), (P, R, V)) in enumerate(zip(hws, geo)):
        lab = torch.empty(h, w, dtype=torch.int32, device=dev)
        _lib.call("unetdc_polygon_fill", ptr(0, i) if P else None, ptr(1, i), ptr(2, i), ptr(3, i) if P else None, P, R, V, h, w,
                  lab.data_ptr(), ws.data_ptr(), ws.numel(), s)
        _lib.call("unetdc_label_census", lab.data_ptr(), h, w, len(uniq[i]), area_d[int(first[i]):].data_ptr(), s)
        labels.append(lab)
    area_h = area_d.cpu().numpy()                                                   # the batch's only host wait
    out, luts = [], []
    for i, u in enumerate(uniq):
        a = area_h[int(first[i]):int(first[i + 1])]
        keep = a > 0
        lut = np.where(keep, np.cumsum(keep), 0) if compact else u
        luts.append(None if np.array_equal(lut, np.arange(1, len(u) + 1)) else lut.astype(np.int32))
        out.append({"labels": labels[i], "kept": u[keep].astype(np.int64), "area": a[keep].astype(np.int64)})
    todo = [i for i, t in enumerate(luts) if t is not None]
    if todo:
        lat = np.concatenate([[0], np.cumsum([len(luts[i]) for i in todo])]).astype(np.int64)
        lut_d = torch.from_numpy(np.concatenate([luts[i] for i in todo])).to(dev)
        for j, i in enumerate(todo):
            _lib.call("unetdc_label_relabel", labels[i].data_ptr(), *hws[i], lut_d[int(lat[j]):].data_ptr(), len(luts[i]), s)
    return out
