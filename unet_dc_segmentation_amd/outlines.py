"""Droplet outlines as polygons on the HIP device (csrc/outlines.hip), behind the droplet stage of
``droplets.py``: it reads the label map that stage returns and the areas of its table, like ``evaluate.py``.

The yardstick is the host restatement ``utils/droplet_outlines.py`` (bit-exact, tests/test_gpu_outlines.py), which also turns the
integers into columns, rings, GeoJSON and COCO.  Per batch every launch is enqueued on the current stream; the host waits once
for the counts of every image and then copies the filled parts of the tables and vertex lists alone.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

NQ, NF = 6, 5                                            # UNETDC_OUTLINE_QUANTITIES, UNETDC_CONTOUR_FIELDS
ROOM_KEYS = ("max_cracks", "max_len", "max_contours", "max_vertices")


def rooms_for(area, connected=True):
    """The rooms of one image from the areas of its droplets: a 4-connected droplet of A pixels has at most 2 A + 2 cracks (4 A
    less two for each of the A - 1 adjacencies of a spanning tree), any label at most 4 A; a contour has at most as many
    vertices as cracks and at least four cracks."""
    a = [int(v) for v in area]
    if connected:
        cracks, longest = sum(2 * v + 2 for v in a), max((2 * v + 2 for v in a), default=0)
    else:
        cracks = longest = 4 * sum(a)
    return {"max_cracks": cracks, "max_len": longest, "max_contours": (cracks + 3) // 4, "max_vertices": cracks}


def _enqueue(labels, ns, rooms, ws, s):
    """The launches of every image, back to back -> (needed int32 [B, 4] on the host, per image the device views rows, contours,
    vx, vy).  One allocation holds every output; the one copy of the counts is the wait."""
    dev = labels[0].device
    n64 = [NQ * n + NF * r["max_contours"] for n, r in zip(ns, rooms)]
    n32 = [2 * r["max_vertices"] for r in rooms]
    o64, o32 = np.concatenate([[0], np.cumsum(n64)]).astype(np.int64), np.concatenate([[4 * len(ns)], 4 * len(ns) + np.cumsum(n32)]).astype(np.int64)
    buf = torch.empty(8 * int(o64[-1]) + 4 * int(o32[-1]), dtype=torch.uint8, device=dev)
    b64, b32 = buf[:8 * int(o64[-1])].view(torch.int64), buf[8 * int(o64[-1]):].view(torch.int32)
    views = []
    for i, (lab, n, r) in enumerate(zip(labels, ns, rooms)):
        h, w = lab.shape
        seg = b64[int(o64[i]):int(o64[i + 1])]
        rows, cont = seg[:NQ * n], seg[NQ * n:]
        mv = r["max_vertices"]
        vx, vy = b32[int(o32[i]):int(o32[i]) + mv], b32[int(o32[i]) + mv:int(o32[i + 1])]
        _lib.call("unetdc_label_outlines", lab.data_ptr(), n, h, w, r["max_len"], ws.data_ptr(), ws.numel(),
                  rows.data_ptr() if n else None, cont.data_ptr() if r["max_contours"] else None, r["max_contours"],
                  vx.data_ptr() if mv else None, vy.data_ptr() if mv else None, mv, r["max_cracks"], b32[4 * i:].data_ptr(), s)
        views.append((rows, cont, vx, vy))
    needed = b32[:4 * len(ns)].cpu().numpy().reshape(len(ns), 4).astype(np.int64)
    return needed, views


def _fits(need, room):
    return need[0] <= room["max_cracks"] and not need[3] and need[1] <= room["max_contours"] and need[2] <= room["max_vertices"]


def label_outlines_batch(labels, areas, rooms=None, connected=True):
    """labels: B int32 [h, w] device label maps as mask_and_droplets_batch(..., return_labels=True) returns them (0 = background,
    droplets 1..n); areas: per image the host array of its n droplet areas, from which the rooms are computed (rooms_for;
    connected=False for labels that need not be 4-connected).  rooms: a dict with ROOM_KEYS, or one per image, instead.  An
    image whose counts exceed a room, or with a contour longer than max_len, is run again alone with the exact rooms.
    -> per image the record of utils.droplet_outlines.outlines_numpy."""
    B = len(labels)
    if len(areas) != B:
        raise _lib.UnetdcError("label_outlines_batch needs one area array per label map")
    if B == 0:
        return []
    for lab in labels:
        if not (torch.is_tensor(lab) and lab.is_cuda and lab.dtype == torch.int32 and lab.dim() == 2 and lab.is_contiguous()):
            raise _lib.UnetdcError("label_outlines_batch needs contiguous [h, w] int32 device label maps")
    ns = [len(a) for a in areas]
    if rooms is None:
        rooms = [rooms_for(a, connected) for a in areas]
    elif isinstance(rooms, dict):
        rooms = [rooms] * B
    if len(rooms) != B or any(set(r) != set(ROOM_KEYS) or min(int(r[k]) for k in ROOM_KEYS) < 0 for r in rooms):
        raise _lib.UnetdcError(f"label_outlines_batch: rooms are non-negative {ROOM_KEYS}, one set per image")
    rooms = [{k: int(r[k]) for k in ROOM_KEYS} for r in rooms]
    recs = _run(list(labels), ns, rooms)
    again = [i for i, (rec, r) in enumerate(zip(recs, rooms)) if not _fits(rec["needed"], r)]
    for i in again:                                      # alone, with room for exactly what the first run counted
        need = recs[i]["needed"]
        cracks = int(need[0])
        listed = cracks <= rooms[i]["max_cracks"] and not need[3]        # then the contours and vertices were counted too
        exact = {"max_cracks": cracks, "max_len": cracks, "max_contours": int(need[1]) if listed else (cracks + 3) // 4,
                 "max_vertices": int(need[2]) if listed else cracks}
        recs[i] = _run([labels[i]], [ns[i]], [exact])[0]
        if not _fits(recs[i]["needed"], exact):
            raise _lib.UnetdcError(f"label_outlines_batch: image {i} does not fit the rooms it asked for ({recs[i]['needed'].tolist()})")
    for rec in recs:
        del rec["needed"]
    return recs


def _run(labels, ns, rooms):
    from utils.droplet_outlines import CONTOUR_FIELDS, QUANTITIES
    lib = _lib.load()
    sizes = [lib.unetdc_label_outlines_workspace(lab.shape[0], lab.shape[1], n, r["max_cracks"]) for lab, n, r in zip(labels, ns, rooms)]
    if min(sizes) <= 0:
        raise _lib.UnetdcError("label_outlines_batch: an image size or a room the library refuses (sides 1..16384, at most 2^30 cracks)")
    ws = torch.empty(max(sizes), dtype=torch.uint8, device=labels[0].device)     # one workspace: the launches are stream-ordered
    needed, views = _enqueue(labels, ns, rooms, ws, torch.cuda.current_stream().cuda_stream)
    parts64, parts32, recs = [], [], []
    for need, (rows, cont, vx, vy), n, r in zip(needed, views, ns, rooms):
        nc, nv = (int(need[1]), int(need[2])) if _fits(need, r) else (0, 0)      # an image that runs again brings its rows alone
        parts64 += [rows] + [cont[f * r["max_contours"]:f * r["max_contours"] + nc] for f in range(NF)]
        parts32 += [vx[:nv], vy[:nv]]
    h64, h32 = torch.cat(parts64).cpu().numpy(), torch.cat(parts32).cpu().numpy()      # the filled parts alone
    a = b = 0
    for need, n, r in zip(needed, ns, rooms):
        nc, nv = (int(need[1]), int(need[2])) if _fits(need, r) else (0, 0)
        rows = h64[a:a + NQ * n].reshape(NQ, n)
        cont = h64[a + NQ * n:a + NQ * n + NF * nc].reshape(NF, nc)
        a += NQ * n + NF * nc
        recs.append({"rows": {q: rows[j].copy() for j, q in enumerate(QUANTITIES)},
                     "contours": {f: cont[j].copy() for j, f in enumerate(CONTOUR_FIELDS)},
                     "x": h32[b:b + nv].copy(), "y": h32[b + nv:b + 2 * nv].copy(), "needed": need})
        b += 2 * nv
    return recs
