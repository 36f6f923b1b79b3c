"""Predicted droplets against annotated masks on the HIP device (csrc/match.hip): the overlap table
of two device label maps through ``unetdc_label_overlap``, and a whole batch of images enqueued back to back.

Only the triples (a, b, n) and three integers per annotated droplet cross PCIe; the decisions and the float64 columns are
``utils.droplet_match.match_columns`` on the host, the same function the CPU path uses.

``sweep_batch`` / ``sweep_result`` (csrc/sweep.hip): the pixel confusion matrix of the thresholded mask
against the annotation at every threshold of a grid, added up in one device histogram for as many images as the caller
likes; ``utils.threshold_sweep.sweep_table`` turns its single copy into the scores.

``boundary_batch`` / ``boundary_result`` (csrc/boundary.hip): the surface distances between the boundary
pixels of predicted and annotated label maps, a batch enqueued back to back; ``utils.droplet_boundary.boundary_columns`` turns
the integers into HD, HD95, ASSD and surface Dice.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def first_capacity(ka, kb):
    """Room for the triples of the first try: droplets are compact, a handful of partners each."""
    return 4 * (int(ka) + int(kb)) + 64


def _check_labels(t, what):
    if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous():
        raise _lib.UnetdcError(f"{what} must be a contiguous int32 [h, w] tensor on the HIP device")


def label_overlap(label_a, ka, label_b, kb, capacity=None):
    """label_a, label_b: int32 [h, w] DEVICE label maps (objects 1..ka, 1..kb).  -> int64 arrays (a, b, n): the overlap table
    in (a, b) order.  The first try has room for first_capacity(ka, kb) triples (or `capacity`); a table that does not fit
    is computed again with four times the room, at most h * w, which always suffices."""
    _check_labels(label_a, "label_a")
    _check_labels(label_b, "label_b")
    if label_a.shape != label_b.shape:
        raise _lib.UnetdcError("the two label maps differ in size")
    h, w = label_a.shape
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    dev = label_a.device
    cap = int(min(max(first_capacity(ka, kb) if capacity is None else int(capacity), 0), h * w))
    while True:
        wsb = lib.unetdc_label_overlap_workspace(h, w, cap)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        out = torch.empty(1 + 3 * cap, dtype=torch.int32, device=dev)
        rows = out[1:].view(3, cap)
        _lib.call("unetdc_label_overlap", label_a.data_ptr(), int(ka), label_b.data_ptr(), int(kb), h, w, ws.data_ptr(), wsb,
                  out.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), cap, s)
        n = int(out[:1].cpu()[0])
        if n <= cap:
            t = rows[:, :n].cpu().numpy().astype(np.int64)
            return t[0], t[1], t[2]
        cap = min(4 * max(cap, 1), h * w)


def match_batch(pred_labels, pred_areas, gts, gt_min_area=1, gt_are_labels=False, max_gt=1 << 14, keep_labels=False):
    """pred_labels: B int32 [h, w] DEVICE label maps; pred_areas: B int64 arrays, the areas of their objects 1..Ka;
    gts: B annotations of the same sizes, numpy arrays or DEVICE tensors -- binary masks (nonzero = droplet; labelled here by
    4-connected components of at least gt_min_area pixels, never split) or, with gt_are_labels, integer label images whose
    values are the labels as they are (areas by bincount on the host; gt_min_area does not apply).
    Every launch of the batch (per image unetdc_ccl_labels, then unetdc_label_overlap) is enqueued back to back on the
    current stream into one set of output planes; the host then waits ONCE, on the copy of the counts, and fetches the
    filled part of the int32 and of the int64 outputs.  An image with more annotated droplets than max_gt, or more pairs
    than its first capacity, is computed again on its own.
    Returns per image a dict: a, b, n (the triples), gt_area, gt_sumy, gt_sumx (int64 [Kb]) and columns =
    utils.droplet_match.match_columns(pred_area, gt_area, a, b, n); with keep_labels also gt_labels, the annotation's int32
    DEVICE label map (objects 1..len(gt_area)), for boundary_batch."""
    from utils.droplet_match import label_sums, match_columns
    B = len(pred_labels)
    if not (len(pred_areas) == len(gts) == B):
        raise _lib.UnetdcError("match_batch needs one area list and one annotation per label map")
    if B == 0:
        return []
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    dev = pred_labels[0].device
    hws, kas = [], [len(a) for a in pred_areas]
    for lab in pred_labels:
        _check_labels(lab, "a predicted label map")
        hws.append((int(lab.shape[0]), int(lab.shape[1])))
    host_sums, gt_dev = [None] * B, []
    for i, g in enumerate(gts):
        if tuple(g.shape) != hws[i]:
            raise _lib.UnetdcError(f"annotation {i} is {tuple(g.shape)}, its image {hws[i]}")
        if gt_are_labels:
            g_h = g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
            if g_h.max(initial=0) > 2 ** 31 - 1:
                raise _lib.UnetdcError("labels above 2^31 - 1")
            host_sums[i] = label_sums(g_h)
            g = g if torch.is_tensor(g) and g.dtype == torch.int32 else torch.from_numpy(np.ascontiguousarray(g_h, dtype=np.int32))
        else:
            g = g if torch.is_tensor(g) else torch.from_numpy(np.ascontiguousarray(np.asarray(g) > 0, dtype=np.uint8))
            g = g if g.dtype == torch.uint8 else (g != 0).to(torch.uint8)
        gt_dev.append(g.to(dev).contiguous())
    capb = 0 if gt_are_labels else int(min(max_gt, max(h * w for h, w in hws)))
    # the number of annotated droplets is not known before the wait: room for as many pairs as twice the prediction suggests
    caps = [int(min(first_capacity(ka, ka) + 1024, h * w)) for ka, (h, w) in zip(kas, hws)]
    P = max(caps)
    wsb = max(max(lib.unetdc_label_overlap_workspace(h, w, c) for (h, w), c in zip(hws, caps)),
              0 if gt_are_labels else max(lib.unetdc_ccl_labels_workspace(h, w) for h, w in hws))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)           # one workspace: the launches are stream-ordered
    counts = torch.zeros(B, 2, dtype=torch.int32, device=dev)      # annotated droplets, triples
    W = max(capb, P, 1)
    i32 = torch.empty(B, 4, W, dtype=torch.int32, device=dev)      # gt area, then a, b, n
    i64 = torch.empty(B, 2, max(capb, 1), dtype=torch.int64, device=dev)
    gt_labels = []
    for i, (h, w) in enumerate(hws):
        if gt_are_labels:
            lab, kb = gt_dev[i], len(host_sums[i][0])
        else:
            lab, kb = torch.empty(h, w, dtype=torch.int32, device=dev), capb
            _lib.call("unetdc_ccl_labels", gt_dev[i].data_ptr(), h, w, int(max(gt_min_area, 1)), ws.data_ptr(), wsb,
                      counts[i, 0:].data_ptr(), i32[i, 0].data_ptr(), i64[i, 0].data_ptr(), i64[i, 1].data_ptr(), None,
                      lab.data_ptr(), capb, s)
        _lib.call("unetdc_label_overlap", pred_labels[i].data_ptr(), kas[i], lab.data_ptr(), kb, h, w, ws.data_ptr(), wsb,
                  counts[i, 1:].data_ptr(), i32[i, 1].data_ptr(), i32[i, 2].data_ptr(), i32[i, 3].data_ptr(), caps[i], s)
        gt_labels.append(lab)
    c = counts.cpu().numpy().astype(np.int64)                      # the batch's only host wait
    filled = int(max(min(c[:, 0].max(initial=0), capb), np.minimum(c[:, 1], caps).max(initial=0)))
    v32 = i32[:, :, :filled].cpu().numpy().astype(np.int64)
    v64 = i64[:, :, :int(min(c[:, 0].max(initial=0), capb))].cpu().numpy()
    out = []
    for i, (h, w) in enumerate(hws):
        lab = gt_labels[i]
        if gt_are_labels:
            area, sy, sx = host_sums[i]
        elif c[i, 0] > capb:                      # more annotated droplets than the outputs hold: this image again with room
            area, sy, sx, lab = _gt_labels_again(lib, gt_dev[i], h, w, gt_min_area, int(c[i, 0]), s)
        else:
            area, sy, sx = v32[i, 0, :c[i, 0]], v64[i, 0, :c[i, 0]], v64[i, 1, :c[i, 0]]
        if c[i, 1] > caps[i] or (not gt_are_labels and c[i, 0] > capb):
            a, b, n = label_overlap(pred_labels[i], kas[i], lab, len(area))
        else:
            a, b, n = (v32[i, j, :c[i, 1]] for j in (1, 2, 3))
        out.append({"a": a, "b": b, "n": n, "gt_area": area, "gt_sumy": sy, "gt_sumx": sx,
                    "columns": match_columns(pred_areas[i], area, a, b, n)})
        if keep_labels:
            out[-1]["gt_labels"] = lab
    return out


def _gt_labels_again(lib, mask, h, w, min_area, k, s):
    dev = mask.device
    wsb = lib.unetdc_ccl_labels_workspace(h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    area = torch.empty(k, dtype=torch.int32, device=dev)
    sums = torch.empty(2, k, dtype=torch.int64, device=dev)
    lab = torch.empty(h, w, dtype=torch.int32, device=dev)
    _lib.call("unetdc_ccl_labels", mask.data_ptr(), h, w, int(max(min_area, 1)), ws.data_ptr(), wsb, count.data_ptr(),
              area.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), None, lab.data_ptr(), k, s)
    s_h = sums.cpu().numpy()
    return area.cpu().numpy().astype(np.int64), s_h[0], s_h[1], lab


def _gt_run(gts, oh, ow, dev):
    """Annotations of one size -> ONE contiguous uint8 [n, oh, ow] device tensor (nonzero = annotated)."""
    if torch.is_tensor(gts):
        g = gts if gts.dtype == torch.uint8 else (gts != 0).to(torch.uint8)
    elif all(not torch.is_tensor(g) for g in gts):                 # host arrays: one upload for the run
        hs = [np.asarray(g) for g in gts]
        g = torch.from_numpy(np.stack([h if h.dtype == np.uint8 else (h != 0).astype(np.uint8) for h in hs]))
    else:
        ts = [g if torch.is_tensor(g) else torch.from_numpy(np.ascontiguousarray(g)) for g in gts]
        g = torch.stack([(t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)).to(dev) for t in ts])
    if tuple(g.shape[1:]) != (oh, ow):
        raise _lib.UnetdcError(f"an annotation is {tuple(g.shape[1:])}, its image {(oh, ow)}")
    return g.to(dev).contiguous()


def sweep_batch(probs, gts, out_hws, K, hist=None, linear=True):
    """probs: [B, H, W] fp32 probabilities on the HIP device; gts: B annotations (numpy arrays or tensors of the output sizes,
    nonzero = annotated; or one [B, oh, ow] tensor); out_hws: B (oh, ow) pairs; K: thresholds k / K, k = 0..K-1.
    One unetdc_thresh_sweep per run of consecutive images with equal output size is enqueued on the current stream; every
    call ADDS into the int64 [2, K + 1] device tensor `hist` (a new zeroed one when None), which is returned.  Nothing waits
    for the device: pool as many batches as you like, then sweep_result(hist) makes the one copy.
    linear=True resizes as the droplet stage does (droplets.MASK_RESIZE: the reference's 8-bit bilinear through the cached
    tables of preprocess.py, the identity at equal sizes); linear=False is the nearest rule."""
    from . import droplets
    if not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 3:
        raise _lib.UnetdcError("sweep_batch needs a [B, H, W] fp32 tensor on the HIP device")
    probs = probs.contiguous()
    B, ph, pw = probs.shape
    K = int(K)
    out_hws = [(int(h), int(w)) for h, w in out_hws]
    if not (len(out_hws) == len(gts) == B):
        raise _lib.UnetdcError("sweep_batch needs one annotation and one output size per probability map")
    dev = probs.device
    if hist is None:
        hist = torch.zeros(2, K + 1, dtype=torch.int64, device=dev)
    elif not hist.is_cuda or hist.dtype != torch.int64 or tuple(hist.shape) != (2, K + 1) or not hist.is_contiguous():
        raise _lib.UnetdcError(f"hist must be a contiguous int64 [2, {K + 1}] tensor on the HIP device")
    s = torch.cuda.current_stream().cuda_stream
    i = 0
    while i < B:
        j = i + 1
        while j < B and out_hws[j] == out_hws[i]:
            j += 1
        oh, ow = out_hws[i]
        g = _gt_run(gts[i:j], oh, ow, dev)
        tables = [None] * 4
        if linear and droplets.MASK_RESIZE != "nearest" and (ph, pw) != (oh, ow):
            from .preprocess import _resize_tables
            xo, xa = _resize_tables(pw, ow, dev, True)
            yo, ya = _resize_tables(ph, oh, dev, False)
            tables = [xo.data_ptr(), xa.data_ptr(), yo.data_ptr(), ya.data_ptr()]
        _lib.call("unetdc_thresh_sweep", probs[i:j].data_ptr(), j - i, ph, pw, g.data_ptr(), oh, ow, *tables, K,
                  hist.data_ptr(), s)
        i = j
    return hist


def sweep_result(hist):
    """The device histogram of sweep_batch -> int64 numpy [2, K + 1]: the sweep's only device-to-host copy."""
    return hist.cpu().numpy()


def boundary_batch(pred_labels, kas, gt_labels, kbs, radius, hist=None, dmax=None, objects=True):
    """pred_labels, gt_labels: B int32 [h, w] DEVICE label maps each (image i of both lists has one size; the sizes may differ
    between images); kas, kbs: B label limits (objects 1..ka, 1..kb; a binary mask is a label map with k = 1); radius: 1..64.
    One unetdc_boundary_distances per image is enqueued back to back on the current stream into ONE workspace and ONE int64
    output plane (histograms, tables and the two maxima); the host then waits ONCE, on the copy of that plane.
    hist (int64 [2, radius^2 + 2]) and dmax (int32 [2], initialised to -1) given, both on the device: every image ADDS into them
    (pool as many batches as you like, then boundary_result(hist, dmax) makes the copy) and nothing is fetched for them; with
    objects False as well nothing waits for the device at all.
    Returns per image the record of utils.droplet_boundary.boundary_record_numpy as int64 arrays: hist, dmax (None when
    pooled), a, b (None without objects)."""
    from utils.droplet_boundary import check_radius
    B, R = len(pred_labels), check_radius(radius)
    if not (len(kas) == len(gt_labels) == len(kbs) == B):
        raise _lib.UnetdcError("boundary_batch needs one label limit per map and one annotation per prediction")
    if (hist is None) != (dmax is None):
        raise _lib.UnetdcError("hist and dmax come together or not at all")
    nb = R * R + 2
    if B == 0:
        return []
    dev = pred_labels[0].device
    if hist is not None:
        if not (hist.is_cuda and hist.dtype == torch.int64 and tuple(hist.shape) == (2, nb) and hist.is_contiguous()):
            raise _lib.UnetdcError(f"hist must be a contiguous int64 [2, {nb}] tensor on the HIP device")
        if not (dmax.is_cuda and dmax.dtype == torch.int32 and tuple(dmax.shape) == (2,) and dmax.is_contiguous()):
            raise _lib.UnetdcError("dmax must be a contiguous int32 [2] tensor on the HIP device")
    hws, kas, kbs = [], [int(k) for k in kas], [int(k) for k in kbs]
    for a, b in zip(pred_labels, gt_labels):
        _check_labels(a, "a predicted label map")
        _check_labels(b, "an annotated label map")
        if a.shape != b.shape:
            raise _lib.UnetdcError("the two label maps differ in size")
        hws.append((int(a.shape[0]), int(a.shape[1])))
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    wsb = max(lib.unetdc_boundary_distances_workspace(h, w) for h, w in hws)
    if min(lib.unetdc_boundary_distances_workspace(h, w) for h, w in hws) <= 0 or min(kas + kbs) < 0:
        raise _lib.UnetdcError("boundary_batch: sides 1..16384, non-negative label limits")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)           # one workspace: the launches are stream-ordered
    pooled = hist is not None
    # one int64 plane: per image [2, nb] histogram (unless pooled), then the tables [3, ka], [3, kb], then B words = [B, 2] int32
    n_hist = 0 if pooled else B * 2 * nb
    offs, at = [], n_hist
    for ka, kb in zip(kas, kbs):
        offs.append((at, at + 3 * ka))
        at += (3 * ka + 3 * kb) if objects else 0
    n_dmax = 0 if pooled else B
    plane = torch.zeros(max(at + n_dmax, 1), dtype=torch.int64, device=dev)
    if n_dmax:
        plane[at:].fill_(-1)                                       # both int32 halves of every word are -1
        dm = plane[at:].view(torch.int32).view(B, 2)
    for i, (h, w) in enumerate(hws):
        oa, ob = offs[i]
        _lib.call("unetdc_boundary_distances", pred_labels[i].data_ptr(), kas[i], gt_labels[i].data_ptr(), kbs[i], h, w, R,
                  ws.data_ptr(), wsb, hist.data_ptr() if pooled else plane[i * 2 * nb:].data_ptr(),
                  dmax.data_ptr() if pooled else dm[i].data_ptr(),
                  plane[oa:].data_ptr() if objects and kas[i] else None, plane[ob:].data_ptr() if objects and kbs[i] else None, s)
    if pooled and not objects:
        return [{"hist": None, "dmax": None, "a": None, "b": None} for _ in range(B)]
    host = plane.cpu().numpy()                                     # the batch's only host wait
    out = []
    for i, (ka, kb) in enumerate(zip(kas, kbs)):
        oa, ob = offs[i]
        out.append({"hist": None if pooled else host[i * 2 * nb:(i + 1) * 2 * nb].reshape(2, nb).copy(),
                    "dmax": None if pooled else host[at + i:at + i + 1].view(np.int32).astype(np.int64),
                    "a": host[oa:oa + 3 * ka].reshape(3, ka).copy() if objects else None,
                    "b": host[ob:ob + 3 * kb].reshape(3, kb).copy() if objects else None})
    return out


def _check_plane(t, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
        raise _lib.UnetdcError(f"{what} must be a contiguous uint8 [h, w] tensor on the HIP device")


def _diff_tables(v32, v64, n):
    """Row j of the int32 planes (class, area, neighbors) and of the int64 planes (sumy, sumx) -> the table of n rows."""
    return {"class": v32[0, :n].astype(np.int64), "area": v32[1, :n].astype(np.int64), "sumy": v64[0, :n].copy(),
            "sumx": v64[1, :n].copy(), "neighbors": v32[2, :n].astype(np.int64)}


def diff_regions_batch(preds, gts, min_area=1, images=None, paint=False, max_regions=1 << 14):
    """preds, gts: B uint8 [h, w] DEVICE planes each (nonzero = set; image i of both lists has one size, the sizes may differ
    between images); images: optionally B uint8 [h, w, 3] DEVICE tensors, the pictures the overlays are painted on.
    Per image unetdc_diff_regions (and with paint unetdc_diff_paint) is enqueued back to back on the current stream into ONE
    workspace and one set of output planes; the host then waits ONCE, on the copy of the twelve image integers and the row
    counts, and fetches the filled part of the tables.  An image with more rows than max_regions is run again alone with room.
    Returns per image the record of utils.difference_map.diff_regions_numpy: image (int64 [12]), class, area, sumy, sumx,
    neighbors (int64 arrays); with paint also diff (uint8 [h, w, 3] DEVICE tensor) and overlay (the same on images[i]; None
    without images)."""
    B = len(preds)
    if len(gts) != B or (images is not None and len(images) != B):
        raise _lib.UnetdcError("diff_regions_batch needs one annotation (and one image, if any) per prediction")
    if B == 0:
        return []
    min_area, max_regions = int(min_area), int(max_regions)
    if min_area < 1 or max_regions < 0:
        raise _lib.UnetdcError("diff_regions_batch: min_area >= 1, max_regions >= 0")
    lib = _lib.load()
    hws = []
    for i, (p, g) in enumerate(zip(preds, gts)):
        _check_plane(p, "a prediction")
        _check_plane(g, "an annotation")
        if p.shape != g.shape:
            raise _lib.UnetdcError(f"annotation {i} is {tuple(g.shape)}, its prediction {tuple(p.shape)}")
        hws.append((int(p.shape[0]), int(p.shape[1])))
        if images is not None:
            im = images[i]
            if not (torch.is_tensor(im) and im.is_cuda and im.dtype == torch.uint8 and tuple(im.shape) == hws[i] + (3,) and
                    im.is_contiguous()):
                raise _lib.UnetdcError(f"image {i} must be a contiguous uint8 {hws[i] + (3,)} tensor on the HIP device")
    sizes = [lib.unetdc_diff_regions_workspace(h, w) for h, w in hws]
    if min(sizes) <= 0:
        raise _lib.UnetdcError("diff_regions_batch: sides 1..16384, h * w < 2^30")
    s = torch.cuda.current_stream().cuda_stream
    dev = preds[0].device
    wsb = max(sizes)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)           # one workspace: the launches are stream-ordered
    cap = int(min(max_regions, max(h * w for h, w in hws)))
    head = torch.zeros(B, 13, dtype=torch.int64, device=dev)       # the twelve image integers, then the row count (int32)
    i32 = torch.empty(B, 3, max(cap, 1), dtype=torch.int32, device=dev)     # class, area, neighbors
    i64 = torch.empty(B, 2, max(cap, 1), dtype=torch.int64, device=dev)     # sumy, sumx
    pics = []
    for i, (h, w) in enumerate(hws):
        tables = [i32[i, 0], i32[i, 1], i64[i, 0], i64[i, 1], i32[i, 2]] if cap else [None] * 5
        _lib.call("unetdc_diff_regions", preds[i].data_ptr(), gts[i].data_ptr(), h, w, min_area, ws.data_ptr(), wsb,
                  head[i].data_ptr(), head[i, 12:].data_ptr(), *(t.data_ptr() if t is not None else None for t in tables), cap, s)
        if paint:
            diff = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
            over = torch.empty(h, w, 3, dtype=torch.uint8, device=dev) if images is not None else None
            _lib.call("unetdc_diff_paint", preds[i].data_ptr(), gts[i].data_ptr(),
                      images[i].data_ptr() if images is not None else None, h, w, diff.data_ptr(),
                      over.data_ptr() if over is not None else None, s)
            pics.append((diff, over))
    host = head.cpu().numpy()                                      # the batch's only host wait
    counts = host[:, 12] & 0xFFFFFFFF                              # the int32 the call wrote into the zeroed word
    filled = int(np.minimum(counts, cap).max(initial=0))
    v32 = i32[:, :, :filled].cpu().numpy()
    v64 = i64[:, :, :filled].cpu().numpy()
    out = []
    for i, (h, w) in enumerate(hws):
        n = int(counts[i])
        if n > cap:                                                # more rows than the planes hold: this image again with room
            rec = _diff_regions_again(preds[i], gts[i], h, w, min_area, n, s)
        else:
            rec = {"image": host[i, :12].copy(), **_diff_tables(v32[i], v64[i], n)}
        if paint:
            rec["diff"], rec["overlay"] = pics[i]
        out.append(rec)
    return out


def _diff_regions_again(pred, gt, h, w, min_area, n, s):
    lib, dev = _lib.load(), pred.device
    wsb = lib.unetdc_diff_regions_workspace(h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    head = torch.zeros(13, dtype=torch.int64, device=dev)
    i32 = torch.empty(3, n, dtype=torch.int32, device=dev)
    i64 = torch.empty(2, n, dtype=torch.int64, device=dev)
    _lib.call("unetdc_diff_regions", pred.data_ptr(), gt.data_ptr(), h, w, min_area, ws.data_ptr(), wsb, head.data_ptr(),
              head[12:].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), i64[0].data_ptr(), i64[1].data_ptr(), i32[2].data_ptr(),
              n, s)
    return {"image": head[:12].cpu().numpy(), **_diff_tables(i32.cpu().numpy(), i64.cpu().numpy(), n)}


def boundary_result(hist, dmax):
    """The pooled device planes of boundary_batch -> (int64 numpy [2, R^2 + 2], int64 numpy [2])."""
    return hist.cpu().numpy(), dmax.cpu().numpy().astype(np.int64)
