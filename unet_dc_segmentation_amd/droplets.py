"""Droplet quantification on the HIP device (csrc/ccl.hip): probabilities -> mask at the original image size -> 4-connected
components -> the per-droplet table of the reference's ``quantify()`` (/root/reference/quantify_droplets_batch.py:81-95).

Only the uint8 mask (needed for the PNG the script writes) and three integers per droplet cross PCIe; the reference
copies every fp32 probability map to the host, labels it twice with scikit-image and walks ``np.unique`` in Python.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def nearest_index(dst, src):
    """Source index of each destination index under cv2.resize(..., INTER_NEAREST): min(floor(d * src / dst), src - 1)."""
    return np.minimum(np.floor(np.arange(dst) * (src / dst)).astype(np.int64), src - 1)


def resize_nearest_cv2(mask, ow, oh):
    """numpy restatement of cv2.resize(mask, (ow, oh), interpolation=cv2.INTER_NEAREST) (used where cv2 is absent)."""
    return mask[nearest_index(oh, mask.shape[0])[:, None], nearest_index(ow, mask.shape[1])[None, :]]


# How the 512 x 512 mask gets to the original image size.  The reference writes
#     cv2.resize(mask512, (ow, oh), cv2.INTER_NEAREST)                    (/root/reference/quantify_droplets_batch.py:57)
# with the flag in the positional slot of `dst`: OpenCV ignores it and runs its default 8-bit INTER_LINEAR on the {0,1} mask.
# "reference" reproduces what that call computes, "nearest" what it names.  (cv2 is not installed here: both rules are
# restatements -- utils/data_loader.py:resize_linear_cv2_u8 and resize_nearest_cv2 below -- parity unpinned against cv2.)
MASK_RESIZE = "reference"


def resize_mask_like_reference(mask, ow, oh):
    """CPU path: uint8 {0,1} mask [h, w] -> [oh, ow] under MASK_RESIZE."""
    if MASK_RESIZE == "nearest" or (mask.shape[0] == oh and mask.shape[1] == ow):
        return resize_nearest_cv2(mask, ow, oh)
    from utils.data_loader import resize_linear_cv2_u8
    return resize_linear_cv2_u8(np.ascontiguousarray(mask, dtype=np.uint8), ow, oh)


def _mask_from_probs(p2, ph, pw, thresh, mask, oh, ow, dev, s):
    """probabilities [ph, pw] > thresh (strict) -> the uint8 mask [oh, ow] under MASK_RESIZE."""
    if MASK_RESIZE == "nearest" or (ph == oh and pw == ow):          # same size: both rules are the identity
        _lib.call("unetdc_mask_from_probs", p2.data_ptr(), ph, pw, float(thresh), mask.data_ptr(), oh, ow, s)
    else:
        from .preprocess import _resize_tables
        xo, xa = _resize_tables(pw, ow, dev, True)
        yo, ya = _resize_tables(ph, oh, dev, False)
        _lib.call("unetdc_mask_from_probs_linear", p2.data_ptr(), ph, pw, float(thresh), mask.data_ptr(), oh, ow,
                  xo.data_ptr(), xa.data_ptr(), yo.data_ptr(), ya.data_ptr(), s)


def _clean_options(thresh, thresh_low, max_hole_area):
    """The mask-cleaning stage of DESIGN.md section 13 -> (low threshold, hole limit), or None when both steps are off (no
    launch is added then).  A low threshold equal to the threshold selects what the threshold selects: off."""
    if thresh_low is not None and not thresh_low <= thresh:
        raise _lib.UnetdcError(f"thresh_low ({thresh_low}) must not exceed thresh ({thresh})")
    low = None if thresh_low is None or thresh_low == thresh else float(thresh_low)
    holes = int(max_hole_area)
    return None if low is None and holes == 0 else (low, holes)


def _clean(clean, mask, p2, ph, pw, oh, ow, ws, wsb, counts_ptr, dev, s):
    """unetdc_mask_clean in place on `mask` (the mask of the threshold): the weak mask is that of the low threshold under
    the same resize rule; the four counts go to counts_ptr."""
    low, holes = clean
    weak = None
    if low is not None:
        weak = torch.empty_like(mask)
        _mask_from_probs(p2, ph, pw, low, weak, oh, ow, dev, s)
    _lib.call("unetdc_mask_clean", mask.data_ptr(), None if weak is None else weak.data_ptr(), oh, ow, holes, ws.data_ptr(), wsb,
              mask.data_ptr(), counts_ptr, s)


def _stats(lib, mask, oh, ow, min_area, ws, wsb, count_ptr, area_ptr, sy_ptr, sx_ptr, cap, s, h2, label):
    """One image's labelling + sums + compaction: unetdc_ccl_stats, or with a split depth (h2 half pixels, not None)
    unetdc_split_stats, which also fills the int32 label plane `label` when one is given."""
    if h2 is None:
        _lib.call("unetdc_ccl_stats", mask.data_ptr(), oh, ow, int(max(min_area, 1)), ws.data_ptr(), wsb, count_ptr, area_ptr,
                  sy_ptr, sx_ptr, None, cap, s)
    else:
        _lib.call("unetdc_split_stats", mask.data_ptr(), oh, ow, int(max(min_area, 1)), h2, ws.data_ptr(), wsb, count_ptr,
                  area_ptr, sy_ptr, sx_ptr, None, None if label is None else label.data_ptr(), cap, s)


def _stats_labels(lib, mask, oh, ow, min_area, ws, wsb, count_ptr, area_ptr, sy_ptr, sx_ptr, cap, s, h2, label, gray, props_ptr):
    """_stats with the label map on either path (unetdc_ccl_labels without a split depth), then unetdc_label_props on
    that map and the optional uint8 grey plane: the shape integers [UNETDC_SHAPE_QUANTITIES][cap] at props_ptr."""
    if h2 is None:
        _lib.call("unetdc_ccl_labels", mask.data_ptr(), oh, ow, int(max(min_area, 1)), ws.data_ptr(), wsb, count_ptr, area_ptr,
                  sy_ptr, sx_ptr, None, label.data_ptr(), cap, s)
    else:
        _stats(lib, mask, oh, ow, min_area, ws, wsb, count_ptr, area_ptr, sy_ptr, sx_ptr, cap, s, h2, label)
    _lib.call("unetdc_label_props", label.data_ptr(), None if gray is None else gray.data_ptr(), oh, ow, props_ptr, cap, s)


def _check_gray(gray, oh, ow):
    if gray is not None and (not gray.is_cuda or gray.dtype != torch.uint8 or tuple(gray.shape) != (oh, ow)
                             or not gray.is_contiguous()):
        raise _lib.UnetdcError("gray must be a contiguous uint8 [oh, ow] tensor on the HIP device")


def _props_dict(area, sumy, sumx, rows, with_gray):
    """The integers utils.droplet_shape.shape_columns reads, under the names of label_props_numpy."""
    from utils.droplet_shape import GRAY_QUANTITIES, QUANTITIES
    out = {"area": area, "Sy": sumy, "Sx": sumx}
    out.update((q, rows[j]) for j, q in enumerate(QUANTITIES) if with_gray or q not in GRAY_QUANTITIES)
    return out


def _ws_query(lib, h2, shape):
    return lib.unetdc_split_workspace if h2 is not None else lib.unetdc_ccl_labels_workspace if shape else lib.unetdc_ccl_workspace


NQ = 14    # UNETDC_SHAPE_QUANTITIES


def _half_pixels(split_depth):
    if split_depth is None:
        return None
    from utils.droplet_split import half_pixels
    return half_pixels(split_depth)


def mask_and_droplets_batch(probs, thresh, out_hws, min_area, max_droplets=1 << 14, keep_sums=False, split_depth=None,
                            return_labels=False, shape=False, gray=None, *, thresh_low=None, max_hole_area=0, clean_counts=None):
    """probs: [B, H, W] fp32 probabilities on the HIP device; out_hws: B (oh, ow) pairs.  Every launch of the batch (mask,
    union-find, per-label sums, compaction) is enqueued back to back on the current stream into ONE set of output
    planes; the host then waits ONCE: one device->host copy brings the B droplet counts, a second the filled part of the
    per-droplet integers.  Returns a list of (mask uint8 [oh, ow] DEVICE tensor, area int64 [n], centroid_row float64
    [n], centroid_col float64 [n]) -- droplets in the reference's label order.  keep_sums=True returns (that list, the
    device outputs (count, area, sumy, sumx) or None when an image had more droplets than they hold) for
    density.density_maps_batch.
    split_depth (pixels, a multiple of 0.5; None = off): touching droplets are cut where the distance transform dips more
    than that below the lower of two peaks (csrc/split.hip, utils/droplet_split.py) -- same launches otherwise, still one
    host wait.  return_labels=True (needs a split depth or shape=True) appends the int32 [oh, ow] DEVICE label map to
    every tuple.
    shape=True appends, last, the dict of per-droplet int64 arrays that utils.droplet_shape.shape_columns reads (area, Sy,
    Sx and the rows of unetdc_label_props); gray: B uint8 [oh, ow] DEVICE tensors (or None: no intensity integers).  The
    label map and the props launches follow each image's existing ones, and the integers travel in the copies the host
    already waits for.
    thresh_low (<= thresh) / max_hole_area (0 = off, negative = any size, N = holes of at most N pixels): the mask is
    cleaned first (hysteresis threshold, hole filling: csrc/clean.hip), and the cleaned mask is the
    one returned, labelled, split and measured.  clean_counts: a list that receives, per image, the int64 [4] counts of
    utils.droplet_clean.COUNT_NAMES; they ride in the copy of the droplet counts.  Both off: no launch is added."""
    h2 = _half_pixels(split_depth)
    clean = _clean_options(thresh, thresh_low, max_hole_area)
    if return_labels and h2 is None and not shape:
        raise _lib.UnetdcError("return_labels needs a split_depth or shape=True")
    if gray is not None and not shape:
        raise _lib.UnetdcError("gray needs shape=True")
    if not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 3:
        raise _lib.UnetdcError("mask_and_droplets_batch needs a [B, H, W] fp32 tensor on the HIP device")
    probs = probs.contiguous()
    B, ph, pw = probs.shape
    dev = probs.device
    s = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    out_hws = [(int(h), int(w)) for h, w in out_hws]
    cap = int(min(max_droplets, max(h * w for h, w in out_hws)))
    if gray is not None:
        for g, (oh, ow) in zip(gray, out_hws):
            _check_gray(g, oh, ow)
    wsb = max(_ws_query(lib, h2, shape)(h, w) for h, w in out_hws)
    if clean is not None:
        wsb = max(wsb, max(lib.unetdc_mask_clean_workspace(h, w) for h, w in out_hws))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)           # one workspace: the launches are stream-ordered
    counts = torch.zeros(B * (1 if clean is None else 5), dtype=torch.int32, device=dev)   # droplet counts, then 4 per image
    count = counts[:B]
    area = torch.empty(B, cap, dtype=torch.int32, device=dev)
    if shape:          # per image: sum y, sum x, then the rows of unetdc_label_props, which wants them [NQ][cap] in one piece
        sums = torch.empty(B, 2 + NQ, cap, dtype=torch.int64, device=dev).permute(1, 0, 2)
    else:
        sums = torch.empty(2, B, cap, dtype=torch.int64, device=dev)
    masks, labels = [], []
    for i, (oh, ow) in enumerate(out_hws):
        mask = torch.empty(oh, ow, dtype=torch.uint8, device=dev)
        label = torch.empty(oh, ow, dtype=torch.int32, device=dev) if return_labels or shape else None
        p2 = probs[i]
        _mask_from_probs(p2, ph, pw, thresh, mask, oh, ow, dev, s)
        if clean is not None:
            _clean(clean, mask, p2, ph, pw, oh, ow, ws, wsb, counts[B + 4 * i:].data_ptr(), dev, s)
        if shape:
            _stats_labels(lib, mask, oh, ow, min_area, ws, wsb, count[i:].data_ptr(), area[i].data_ptr(), sums[0, i].data_ptr(),
                          sums[1, i].data_ptr(), cap, s, h2, label, None if gray is None else gray[i], sums[2, i].data_ptr())
        else:
            _stats(lib, mask, oh, ow, min_area, ws, wsb, count[i:].data_ptr(), area[i].data_ptr(), sums[0, i].data_ptr(),
                   sums[1, i].data_ptr(), cap, s, h2, label)
        masks.append(mask)
        labels.append(label)
    n = counts.cpu().numpy().astype(np.int64)                       # the batch's only host wait
    if clean_counts is not None:
        clean_counts.extend(n[B:].reshape(B, 4) if clean is not None else np.zeros((B, 4), np.int64))
    n = n[:B]
    nmax = int(min(n.max(initial=0), cap))
    a_h = area[:, :nmax].cpu().numpy().astype(np.int64)
    s_h = sums[:, :, :nmax].cpu().numpy()
    out = []
    for i, (oh, ow) in enumerate(out_hws):
        if n[i] > cap:                            # more droplets than the output capacity: this image again with room for all
            out.append(mask_and_droplets(probs[i], thresh, (oh, ow), min_area, max_droplets=int(n[i]), split_depth=split_depth,
                                         return_labels=return_labels, shape=shape, gray=None if gray is None else gray[i],
                                         thresh_low=thresh_low, max_hole_area=max_hole_area))
            continue
        a = a_h[i, :n[i]]
        d = np.maximum(a, 1)
        out.append((masks[i], a, s_h[0, i, :n[i]].astype(np.float64) / d, s_h[1, i, :n[i]].astype(np.float64) / d)
                   + ((labels[i],) if return_labels else ())
                   + ((_props_dict(a, s_h[0, i, :n[i]], s_h[1, i, :n[i]], s_h[2:, i, :n[i]], gray is not None),) if shape else ()))
    if keep_sums:
        return out, ((count, area, sums[0], sums[1]) if n.max(initial=0) <= cap else None)
    return out


def mask_and_droplets(probs2d, thresh, out_hw, min_area, max_droplets=1 << 16, split_depth=None, return_labels=False,
                      shape=False, gray=None, *, thresh_low=None, max_hole_area=0, clean_counts=None):
    """probs2d: [H, W] fp32 probabilities on the HIP device.  Returns (mask uint8 [oh, ow] DEVICE tensor,
    area int64 [n], centroid_row float64 [n], centroid_col float64 [n]) -- droplets in the reference's label order.
    split_depth / return_labels / shape / gray (one uint8 [oh, ow] DEVICE tensor) / thresh_low / max_hole_area: as in
    mask_and_droplets_batch; clean_counts receives this image's int64 [4] counts."""
    h2 = _half_pixels(split_depth)
    clean = _clean_options(thresh, thresh_low, max_hole_area)
    if return_labels and h2 is None and not shape:
        raise _lib.UnetdcError("return_labels needs a split_depth or shape=True")
    if gray is not None and not shape:
        raise _lib.UnetdcError("gray needs shape=True")
    if not probs2d.is_cuda or probs2d.dtype != torch.float32:
        raise _lib.UnetdcError("mask_and_droplets needs an fp32 tensor on the HIP device")
    probs2d = probs2d.contiguous()
    ph, pw = probs2d.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    dev = probs2d.device
    s = torch.cuda.current_stream().cuda_stream
    mask = torch.empty(oh, ow, dtype=torch.uint8, device=dev)
    _mask_from_probs(probs2d, ph, pw, thresh, mask, oh, ow, dev, s)
    lib = _lib.load()
    _check_gray(gray, oh, ow)
    nbytes = _ws_query(lib, h2, shape)(oh, ow)
    if clean is not None:
        nbytes = max(nbytes, lib.unetdc_mask_clean_workspace(oh, ow))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cap = int(min(max_droplets, oh * ow))
    counts = torch.zeros(1 if clean is None else 5, dtype=torch.int32, device=dev)       # droplet count, then the clean counts
    count = counts[:1]
    if clean is not None:
        _clean(clean, mask, probs2d, ph, pw, oh, ow, ws, nbytes, counts[1:].data_ptr(), dev, s)
    area = torch.empty(cap, dtype=torch.int32, device=dev)
    sy = torch.empty(cap, dtype=torch.int64, device=dev)
    sx = torch.empty(cap, dtype=torch.int64, device=dev)
    label = torch.empty(oh, ow, dtype=torch.int32, device=dev) if return_labels or shape else None
    if shape:
        rows = torch.empty(NQ, cap, dtype=torch.int64, device=dev)
        _stats_labels(lib, mask, oh, ow, min_area, ws, nbytes, count.data_ptr(), area.data_ptr(), sy.data_ptr(), sx.data_ptr(),
                      cap, s, h2, label, gray, rows.data_ptr())
    else:
        _stats(lib, mask, oh, ow, min_area, ws, nbytes, count.data_ptr(), area.data_ptr(), sy.data_ptr(), sx.data_ptr(), cap, s,
               h2, label)
    if clean is None:
        n, cc = int(count.item()), np.zeros(4, np.int64)
    else:                                         # one copy brings both
        c_h = counts.cpu().numpy().astype(np.int64)
        n, cc = int(c_h[0]), c_h[1:]
    if n > cap:                                   # more droplets than the output capacity: run again with room for all
        return mask_and_droplets(probs2d, thresh, out_hw, min_area, max_droplets=n, split_depth=split_depth,
                                 return_labels=return_labels, shape=shape, gray=gray, thresh_low=thresh_low,
                                 max_hole_area=max_hole_area, clean_counts=clean_counts)
    if clean_counts is not None:
        clean_counts.append(cc)
    a = area[:n].cpu().numpy().astype(np.int64)
    sy_h, sx_h = sy[:n].cpu().numpy(), sx[:n].cpu().numpy()
    cy = sy_h.astype(np.float64) / np.maximum(a, 1)
    cx = sx_h.astype(np.float64) / np.maximum(a, 1)
    out = (mask, a, cy, cx) + ((label,) if return_labels else ())
    if shape:
        out += (_props_dict(a, sy_h, sx_h, rows[:, :n].cpu().numpy(), gray is not None),)
    return out
