"""Droplet quantification on the HIP device (csrc/ccl.hip): probabilities -> mask at the original image size -> 4-connected
components -> the per-droplet table of the reference's ``quantify()`` (/root/reference/quantify_droplets_batch.py:81-95).

Only the uint8 mask (needed for the PNG the script writes) and three integers per droplet cross PCIe; the reference
copies every fp32 probability map to the host, labels it twice with scikit-image and walks ``np.unique`` in Python.
"""
from __future__ import annotations

import dataclasses
from typing import NamedTuple

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


def _mask_from_probs(p2, thresh, mask, s):
    """probabilities [ph, pw] > thresh (strict) -> the uint8 mask [oh, ow] under MASK_RESIZE."""
    (ph, pw), (oh, ow) = p2.shape, mask.shape
    if MASK_RESIZE == "nearest" or (ph == oh and pw == ow):          # same size: both rules are the identity
        _lib.call("unetdc_mask_from_probs", p2.data_ptr(), ph, pw, float(thresh), mask.data_ptr(), oh, ow, s)
    else:
        from .preprocess import _resize_tables
        xo, xa = _resize_tables(pw, ow, p2.device, True)
        yo, ya = _resize_tables(ph, oh, p2.device, False)
        _lib.call("unetdc_mask_from_probs_linear", p2.data_ptr(), ph, pw, float(thresh), mask.data_ptr(), oh, ow,
                  xo.data_ptr(), xa.data_ptr(), yo.data_ptr(), ya.data_ptr(), s)


@dataclasses.dataclass(frozen=True)
class DropletOptions:
    """What the droplet stage does beyond the plain table, validated where it is built (UnetdcError).
    split_depth (pixels, a multiple of 0.5; None = off): touching droplets are cut where the distance transform dips more
    than that below the lower of two peaks (csrc/split.hip, utils/droplet_split.py).
    shape: also the per-droplet integers that utils.droplet_shape.shape_columns reads (csrc/shape.hip).
    labels: also the int32 label map; needs a split depth, shape, neighbors, confidence or hull.
    thresh_low (<= thresh) / max_hole_area (0 = off, negative = any size, N = holes of at most N pixels): the mask is
    cleaned first (hysteresis threshold, hole filling: csrc/clean.hip).
    neighbors (contact radius in pixels, an integer 1..64; None = off): also the contact pairs and the per-droplet nearest
    contact, degree and cluster (csrc/neighbors.hip, utils/droplet_neighbors.py).
    confidence (the uncertainty band, 0..0.5; None = off): also the per-droplet and per-image integers of the quantised
    probability, its entropy and, given envelope=(lo, hi), the disagreement of the TTA variants (csrc/confidence.hip,
    utils/droplet_confidence.py); confidence_maps: also the uint8 entropy and spread maps, on the device.
    hull: also the per-droplet integers of the convex hull that utils.droplet_hull.hull_columns reads (csrc/hull.hip, DESIGN.md
    section 24).
    thresh / gray are not kept: the threshold the low one is checked against, and the grey planes, which need shape."""
    split_depth: float | None = None
    shape: bool = False
    labels: bool = False
    thresh_low: float | None = None
    max_hole_area: int = 0
    neighbors: int | None = None
    confidence: float | None = None
    confidence_maps: bool = False
    hull: bool = False
    thresh: dataclasses.InitVar[float | None] = None
    gray: dataclasses.InitVar[object] = None

    def __post_init__(self, thresh, gray):
        if self.labels and self.split_depth is None and not self.shape and self.neighbors is None and self.confidence is None and not self.hull:
            raise _lib.UnetdcError("return_labels needs a split_depth or shape=True")
        if self.neighbors is not None:
            from utils.droplet_neighbors import check_radius
            try:
                check_radius(self.neighbors)
            except ValueError as e:
                raise _lib.UnetdcError(str(e)) from None
        if self.confidence is not None:
            from utils.droplet_confidence import check_band
            try:
                check_band(self.confidence)
            except ValueError as e:
                raise _lib.UnetdcError(str(e)) from None
        elif self.confidence_maps:
            raise _lib.UnetdcError("confidence_maps needs confidence (the band)")
        if gray is not None and not self.shape:
            raise _lib.UnetdcError("gray needs shape=True")
        if thresh is not None:
            self.cleaning(thresh)

    @property
    def label_map(self):
        """Whether a stage reads the int32 label map (without a split depth that selects unetdc_ccl_labels)."""
        return self.shape or self.neighbors is not None or self.confidence is not None or self.hull

    @property
    def half_pixels(self):
        if self.split_depth is None:
            return None
        from utils.droplet_split import half_pixels
        return half_pixels(self.split_depth)

    def cleaning(self, thresh):
        """-> (low threshold or None, hole limit), or None when both steps are off (no launch is added then).  A low
        threshold equal to the threshold selects what the threshold selects: off."""
        if self.thresh_low is not None and not self.thresh_low <= thresh:
            raise _lib.UnetdcError(f"thresh_low ({self.thresh_low}) must not exceed thresh ({thresh})")
        low = None if self.thresh_low is None or self.thresh_low == thresh else float(self.thresh_low)
        holes = int(self.max_hole_area)
        return None if low is None and holes == 0 else (low, holes)


def _options(keywords, thresh):
    """The option keywords of the public functions -> (the record, validated against this call's threshold and grey planes;
    gray).  options=DropletOptions(...), or its fields by name (labels also under its earlier name return_labels)."""
    kw = dict(keywords)
    gray, base, envelope = kw.pop("gray", None), kw.pop("options", None) or DropletOptions(), kw.pop("envelope", None)
    if "return_labels" in kw:
        kw["labels"] = kw.pop("return_labels")
    opts = dataclasses.replace(base, **kw, thresh=thresh, gray=gray)
    if envelope is not None and opts.confidence is None:
        raise _lib.UnetdcError("envelope needs confidence (the band)")
    return opts, gray, envelope


@dataclasses.dataclass(eq=False)
class Droplets:
    """One image's result.  Iterates as (mask, area, centroid_row, centroid_col); the rest is reached by name.
    mask: uint8 [oh, ow] DEVICE tensor; area int64 [n], centroid_row / centroid_col float64 [n]: droplets in the
    reference's label order; labels: int32 [oh, ow] DEVICE label map (None unless asked for); props: the dict of
    per-droplet int64 arrays that utils.droplet_shape.shape_columns reads (None without shape); clean_counts: int64 [4],
    the counts of utils.droplet_clean.COUNT_NAMES (zeros when cleaning is off); neighbors: the record of
    utils.droplet_neighbors.neighbors_numpy, int64 arrays (None unless asked for); confidence: the record of
    utils.droplet_confidence.confidence_numpy (None unless asked for), its two maps DEVICE tensors; hull: the dict of five int64
    arrays that utils.droplet_hull.hull_columns reads (None unless asked for).  The CPU path of the script fills the same record
    with host arrays."""
    mask: object
    area: np.ndarray
    centroid_row: np.ndarray
    centroid_col: np.ndarray
    labels: object = None
    props: dict | None = None
    clean_counts: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(4, np.int64))
    neighbors: dict | None = None
    confidence = None             # set by name after construction: the constructor's fields stay those of the stages before
    hull = None                   # likewise

    def __iter__(self):
        return iter((self.mask, self.area, self.centroid_row, self.centroid_col))


class _Image(NamedTuple):
    """One image's views into the batch's buffers."""
    probs: torch.Tensor           # fp32 [ph, pw]
    mask: torch.Tensor            # uint8 [oh, ow]
    label: torch.Tensor | None    # int32 [oh, ow]
    gray: torch.Tensor | None     # uint8 [oh, ow]
    count: torch.Tensor           # int32, the droplet count first
    area: torch.Tensor            # int32 [cap]
    sums: torch.Tensor            # int64 [2 or 2 + NQ, cap]: sum y, sum x, then the rows of unetdc_label_props
    clean_counts: torch.Tensor | None   # int32, the four counts first
    pair_count: torch.Tensor | None = None     # int32, the number of contact pairs first
    pairs: torch.Tensor | None = None          # int32 [3, pair room]: a, b, d2
    per_label: torch.Tensor | None = None      # int32 [5, cap]: the rows of utils.droplet_neighbors.COLUMN_NAMES
    conf: tuple | None = None                  # confidence: (lo, hi fp32 [ph, pw] or None, int64 [8] image totals, the two uint8 maps or None)
    hull_rows: torch.Tensor | None = None      # int32, the row-extent slots unetdc_label_hull needed first


def _enqueue(im, thresh, min_area, ws, opts, s, row_room=0):
    """One image's launches on the stream s: the mask of the threshold; unetdc_mask_clean in place on it (the weak
    mask is that of the low threshold under the same resize rule); labelling + sums + compaction by unetdc_ccl_stats,
    with a split depth unetdc_split_stats (which also fills the label map when there is one), with shape and no split
    depth unetdc_ccl_labels (so does neighbors); then with shape unetdc_label_props on the label map and the optional grey
    plane; then with neighbors unetdc_label_neighbors on the label map, the droplet capacity as its max_label; then with
    confidence unetdc_label_confidence on the label map and the probabilities (and the envelope), the capacity as its max_out,
    into the rows of `sums` behind those of shape; then with hull unetdc_label_hull on the label map, the capacity as its max_out
    and `row_room` row-extent slots, into the rows of `sums` behind those."""
    (oh, ow), cap, h2, clean = im.mask.shape, im.area.shape[0], opts.half_pixels, opts.cleaning(thresh)
    _mask_from_probs(im.probs, thresh, im.mask, s)
    if clean is not None:
        low, holes = clean
        weak = None
        if low is not None:
            weak = torch.empty_like(im.mask)
            _mask_from_probs(im.probs, low, weak, s)
        _lib.call("unetdc_mask_clean", im.mask.data_ptr(), None if weak is None else weak.data_ptr(), oh, ow, holes, ws.data_ptr(),
                  ws.numel(), im.mask.data_ptr(), im.clean_counts.data_ptr(), s)
    head = (im.mask.data_ptr(), oh, ow, int(max(min_area, 1)))
    outs = (ws.data_ptr(), ws.numel(), im.count.data_ptr(), im.area.data_ptr(), im.sums[0].data_ptr(), im.sums[1].data_ptr(), None)
    label = None if im.label is None else im.label.data_ptr()
    if h2 is not None:
        _lib.call("unetdc_split_stats", *head, h2, *outs, label, cap, s)
    elif opts.label_map:
        _lib.call("unetdc_ccl_labels", *head, *outs, label, cap, s)
    else:
        _lib.call("unetdc_ccl_stats", *head, *outs, cap, s)
    if opts.shape:
        _lib.call("unetdc_label_props", label, None if im.gray is None else im.gray.data_ptr(), oh, ow, im.sums[2].data_ptr(), cap, s)
    if opts.neighbors is not None:
        room = im.pairs.shape[1]
        _lib.call("unetdc_label_neighbors", label, cap, oh, ow, int(opts.neighbors), ws.data_ptr(), ws.numel(), im.pair_count.data_ptr(),
                  *((im.pairs[j].data_ptr() if room else None) for j in range(3)), room, *(im.per_label[j].data_ptr() for j in range(5)), s)
    if opts.confidence is not None:
        lo, hi, totals, emap, smap = im.conf
        ph, pw = im.probs.shape
        _lib.call("unetdc_label_confidence", label, cap, oh, ow, im.probs.data_ptr(), *(None if t is None else t.data_ptr() for t in (lo, hi)),
                  ph, pw, float(thresh), float(opts.confidence), _entropy_table(im.probs.device).data_ptr(),
                  im.sums[2 + NQ * opts.shape].data_ptr(), totals.data_ptr(), *(None if t is None else t.data_ptr() for t in (emap, smap)), s)
    if opts.hull:
        _lib.call("unetdc_label_hull", label, cap, oh, ow, ws.data_ptr(), ws.numel(),
                  im.sums[2 + NQ * opts.shape + NC * (opts.confidence is not None)].data_ptr(), im.hull_rows.data_ptr(), row_room, s)


_tables = {}


def _entropy_table(device):
    """utils.droplet_confidence.entropy_table on the device, uploaded once per device (128 KB; int16 holds the uint16 bits)."""
    key = str(device)
    if key not in _tables:
        from utils.droplet_confidence import entropy_table
        _tables[key] = torch.from_numpy(entropy_table().view(np.int16).copy()).to(device)
    return _tables[key]


def _check_gray(gray, oh, ow):
    if not gray.is_cuda or gray.dtype != torch.uint8 or tuple(gray.shape) != (oh, ow) or not gray.is_contiguous():
        raise _lib.UnetdcError("gray must be a contiguous uint8 [oh, ow] tensor on the HIP device")


def _props_dict(area, sums, with_gray):
    """The integers utils.droplet_shape.shape_columns reads, under the names of label_props_numpy."""
    from utils.droplet_shape import GRAY_QUANTITIES, QUANTITIES
    out = {"area": area, "Sy": sums[0], "Sx": sums[1]}
    out.update((q, sums[2 + j]) for j, q in enumerate(QUANTITIES) if with_gray or q not in GRAY_QUANTITIES)
    return out


def _neighbors_dict(pairs, per_label):
    """The record of utils.droplet_neighbors.neighbors_numpy from the int64 copies [3, pairs] and [5, droplets]."""
    from utils.droplet_neighbors import COLUMN_NAMES
    return {"pairs": dict(zip(("a", "b", "d2"), pairs)), **dict(zip(COLUMN_NAMES, per_label))}


def _confidence_dict(rows, totals, envelope, maps):
    """The record of utils.droplet_confidence.confidence_numpy from the int64 copies [NC, droplets] and [8]."""
    from utils.droplet_confidence import CONF_QUANTITIES
    return {**dict(zip(CONF_QUANTITIES, rows)), "image": totals, "envelope": envelope, "entropy_u8": maps[0], "spread_u8": maps[1]}


def _workspace_bytes(lib, out_hws, opts, clean, cap, pair_room, row_room=0):
    query = (lib.unetdc_split_workspace if opts.split_depth is not None else
             lib.unetdc_ccl_labels_workspace if opts.label_map else lib.unetdc_ccl_workspace)
    nbytes = max(query(h, w) for h, w in out_hws)
    if opts.neighbors is not None:
        nbytes = max(nbytes, max(lib.unetdc_label_neighbors_workspace(h, w, cap, pair_room) for h, w in out_hws))
    if clean is not None:
        nbytes = max(nbytes, max(lib.unetdc_mask_clean_workspace(h, w) for h, w in out_hws))
    if opts.hull:
        nbytes = max(nbytes, max(lib.unetdc_label_hull_workspace(h, w, cap, row_room) for h, w in out_hws))
    return nbytes


HULL_QUANTITIES = ("H2", "F2", "Wc", "Wl", "nv")    # the rows of unetdc_label_hull, as utils.droplet_hull.QUANTITIES names them
NQ = 14    # UNETDC_SHAPE_QUANTITIES
NC = 10    # UNETDC_CONF_QUANTITIES
NH = 5     # UNETDC_HULL_QUANTITIES
# Row-extent slots per droplet of the capacity that the first launch of unetdc_label_hull has room for.  The slots needed are the
# sum of the droplets' heights.  The droplets of the flow are connected, so that sum is at most h * w, and the room is capped
# there: then it always suffices.  Below the cap, 64 rows per droplet is three times the about 20 rows of a median droplet of a
# 1040 x 1388 micrograph and 512 KB of workspace per 1024 droplets; an image of taller droplets than that is run again with
# twice the room, like one with more contact pairs than the pair lists hold.
ROWS_PER_DROPLET = 64
PAIR_ROOM = 1 << 14    # contact pairs per image the first launch has room for; an image with more is run again with twice that
MAX_PAIR_ROOM = 1 << 27   # the largest table of unetdc_label_neighbors


def _pair_room(cap, wanted):
    """The pair capacity for a droplet capacity: cap labels have at most cap (cap - 1) / 2 pairs."""
    return int(min(wanted, cap * (cap - 1) // 2, MAX_PAIR_ROOM))


def _row_room(cap, out_hws, wanted=None):
    """The row-extent room of unetdc_label_hull: `wanted` slots (default ROWS_PER_DROPLET per droplet of the capacity), at most
    h * w of the largest image -- the sum of the heights of connected droplets cannot pass that."""
    return int(min(ROWS_PER_DROPLET * cap if wanted is None else wanted, max(h * w for h, w in out_hws)))


def _droplets(probs, thresh, out_hws, min_area, max_droplets, gray, opts, pair_room=None, envelope=None, row_room=None):
    """The one launch-and-readback body -> (B Droplets, the device outputs (count, area, sumy, sumx) or None when an image
    had more droplets than they hold).  Every launch of the batch is enqueued back to back on the current stream into ONE
    set of output planes; the host then waits ONCE: one device->host copy brings the B droplet counts (and the clean
    counts and with neighbors the pair counts behind them), two more the filled part of the per-droplet integers; with
    neighbors one more the per-droplet neighbour integers and one the filled part of the pair lists.  The integers of confidence
    add no copy: the per-droplet rows lie behind the sums, the per-image totals (int64) behind the counts.  Nor do those of hull:
    its rows lie behind those of confidence, the row-extent slots each image needed behind the pair counts."""
    if not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 3:
        raise _lib.UnetdcError("mask_and_droplets_batch needs a [B, H, W] fp32 tensor on the HIP device")
    probs = probs.contiguous()
    if envelope is not None:
        if len(envelope) != 2 or any(not torch.is_tensor(t) or t.dtype != torch.float32 or t.shape != probs.shape or t.device != probs.device
                                     for t in envelope):
            raise _lib.UnetdcError("envelope is (lo, hi): two fp32 tensors shaped like probs, on its device")
        envelope = tuple(t.contiguous() for t in envelope)
    B, dev, s = probs.shape[0], probs.device, torch.cuda.current_stream().cuda_stream
    clean = opts.cleaning(thresh)
    out_hws = [(int(h), int(w)) for h, w in out_hws]
    cap = int(min(max_droplets, max(h * w for h, w in out_hws)))
    if gray is not None:
        for g, (oh, ow) in zip(gray, out_hws):
            _check_gray(g, oh, ow)
    nb = opts.neighbors is not None
    room = _pair_room(cap, PAIR_ROOM if pair_room is None else pair_room) if nb else 0
    rows = _row_room(cap, out_hws, row_room) if opts.hull else 0
    ws = torch.empty(_workspace_bytes(_lib.load(), out_hws, opts, clean, cap, room, rows), dtype=torch.uint8, device=dev)   # one: stream order
    nc, cf, hl = B * (1 if clean is None else 5), opts.confidence is not None, bool(opts.hull)
    n32 = nc + B * nb + B * hl
    at64 = (n32 + 1) // 2 * 2                                          # the int64 totals start on an 8-byte boundary
    # droplet counts, then 4 per image, then the pair counts, then the hull's row counts; then with confidence 8 int64 per image
    # (16 int32 slots)
    counts = torch.zeros(at64 + 16 * B if cf else n32, dtype=torch.int32, device=dev)
    totals = counts[at64:].view(torch.int64) if cf else None
    pairs = torch.empty(B, 3, room, dtype=torch.int32, device=dev) if nb else None
    per_label = torch.empty(B, 5, cap, dtype=torch.int32, device=dev) if nb else None
    area = torch.empty(B, cap, dtype=torch.int32, device=dev)
    # per image: sum y, sum x, then with shape the rows of unetdc_label_props, which wants them [NQ][cap] in one piece
    # and with confidence behind them the rows of unetdc_label_confidence, [NC][cap] in one piece as well, then those of
    # unetdc_label_hull, [NH][cap]
    r0 = 2 + NQ * opts.shape
    rh = r0 + NC * cf
    sums = torch.empty(B, rh + NH * hl, cap, dtype=torch.int64, device=dev).permute(1, 0, 2)
    images = []
    for i, (oh, ow) in enumerate(out_hws):
        images.append(_Image(probs[i], torch.empty(oh, ow, dtype=torch.uint8, device=dev),
                             torch.empty(oh, ow, dtype=torch.int32, device=dev) if opts.labels or opts.label_map else None,
                             None if gray is None else gray[i], counts[i:], area[i], sums[:, i],
                             None if clean is None else counts[B + 4 * i:],
                             *((counts[nc + i:], pairs[i], per_label[i]) if nb else (None, None, None)),
                             (*((envelope[0][i], envelope[1][i]) if envelope is not None else (None, None)), totals[8 * i:],
                              torch.empty(oh, ow, dtype=torch.uint8, device=dev) if opts.confidence_maps else None,
                              torch.empty(oh, ow, dtype=torch.uint8, device=dev) if opts.confidence_maps and envelope is not None else None)
                             if cf else None, counts[nc + B * nb + i:] if hl else None))
        _enqueue(images[i], thresh, min_area, ws, opts, s, rows)
    raw = counts.cpu().numpy()                                      # the batch's only host wait
    t_h = raw[at64:].view(np.int64).reshape(B, 8) if cf else None
    n = raw[:n32].astype(np.int64)
    clean_counts = n[B:nc].reshape(B, 4) if clean is not None else np.zeros((B, 4), np.int64)
    n_pairs, n_rows, n = n[nc:nc + B * nb], n[nc + B * nb:], n[:B]
    nmax = int(min(n.max(initial=0), cap))
    a_h = area[:, :nmax].cpu().numpy().astype(np.int64)
    s_h = sums[:, :, :nmax].cpu().numpy()
    if nb:
        l_h = per_label[:, :, :nmax].cpu().numpy().astype(np.int64)
        p_h = pairs[:, :, :int(min(n_pairs.max(initial=0), room))].cpu().numpy().astype(np.int64)
    out = []
    def again(i, max_droplets, pair_room, row_room):
        return _droplets(probs[i:i + 1], thresh, out_hws[i:i + 1], min_area, max_droplets, None if gray is None else gray[i:i + 1], opts,
                         pair_room, None if envelope is None else tuple(t[i:i + 1] for t in envelope), row_room)[0][0]

    for i, im in enumerate(images):
        if n[i] > cap:                            # more droplets than the output capacity: this image again with room for all
            out.append(again(i, int(n[i]), pair_room, row_room))
            continue
        if nb and n_pairs[i] > room:              # more contact pairs than the pair lists hold: this image again with twice the room
            if room >= MAX_PAIR_ROOM:
                raise _lib.UnetdcError(f"more than {MAX_PAIR_ROOM} contact pairs in one image")
            out.append(again(i, max_droplets, 2 * max(room, 1), row_room))
            continue
        if hl and n_rows[i] > rows:               # taller droplets than the row room holds: this image again with twice the room
            if rows >= out_hws[i][0] * out_hws[i][1]:
                raise _lib.UnetdcError("unetdc_label_hull: connected droplets need more row room than the image has pixels")
            out.append(again(i, max_droplets, pair_room, 2 * max(rows, 1)))
            continue
        a, si = a_h[i, :n[i]], s_h[:, i, :n[i]]
        d = np.maximum(a, 1)
        out.append(Droplets(im.mask, a, si[0].astype(np.float64) / d, si[1].astype(np.float64) / d,
                            im.label if opts.labels else None, _props_dict(a, si, gray is not None) if opts.shape else None,
                            clean_counts[i], _neighbors_dict(p_h[i, :, :n_pairs[i]], l_h[i, :, :n[i]]) if nb else None))
        if cf:
            out[-1].confidence = _confidence_dict(si[r0:r0 + NC], t_h[i], envelope is not None, im.conf[3:])
        if hl:
            out[-1].hull = dict(zip(HULL_QUANTITIES, si[rh:rh + NH]))
    return out, ((counts[:B], area, sums[0], sums[1]) if n.max(initial=0) <= cap else None)


def mask_and_droplets_batch(probs, thresh, out_hws, min_area, max_droplets=1 << 14, keep_sums=False, **options):
    """probs: [B, H, W] fp32 probabilities on the HIP device; out_hws: B (oh, ow) pairs -> a list of B Droplets, after
    ONE host wait for the whole batch (_droplets).  keep_sums=True returns (that list, the device outputs (count, area,
    sumy, sumx) or None when an image had more droplets than they hold) for density.density_maps_batch.
    options: split_depth, shape, return_labels, thresh_low, max_hole_area, neighbors, confidence, confidence_maps, hull by name, or
    options=DropletOptions(...); gray=B uint8 [oh, ow] DEVICE tensors for the intensity integers of shape (None: none); and
    envelope=(lo, hi), two fp32 DEVICE tensors shaped like probs (tta.predict_tta(..., envelope=True)), for the disagreement
    integers of confidence (None: those keep their initial values).  Every option adds its launches
    behind each image's existing ones and its integers to the copies the host already waits for; all off: no launch is added."""
    opts, gray, envelope = _options(options, thresh)
    out, sums = _droplets(probs, thresh, out_hws, min_area, max_droplets, gray, opts, envelope=envelope)
    return (out, sums) if keep_sums else out


def mask_and_droplets(probs2d, thresh, out_hw, min_area, max_droplets=1 << 16, **options):
    """probs2d: [H, W] fp32 probabilities on the HIP device -> its Droplets: the batch of one.  options as in
    mask_and_droplets_batch; gray: one uint8 [oh, ow] DEVICE tensor; envelope: two fp32 [H, W] DEVICE tensors."""
    opts, gray, envelope = _options(options, thresh)
    return _droplets(probs2d[None], thresh, [out_hw], min_area, max_droplets, None if gray is None else [gray], opts,
                     envelope=None if envelope is None else tuple(t[None] for t in envelope))[0][0]
