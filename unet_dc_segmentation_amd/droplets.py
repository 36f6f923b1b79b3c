"""Droplet quantification on the HIP device (csrc/ccl.hip): probabilities -> mask at the original image size -> 4-connected
components -> the per-droplet table of the reference's ``quantify()`` (/root/reference/quantify_droplets_batch.py:81-95).

Only the uint8 mask (needed for the PNG the script writes) and three integers per droplet cross PCIe; the reference
copies every fp32 probability map to the host, labels it twice with scikit-image and walks ``np.unique`` in Python.

Shape: DropletOptions in, one Droplets per image out, one launch-and-readback body (_droplets).  What runs before a label
map exists (mask, cleaning, the choice of labelling kernel) is the explicit head of _enqueue; every optional stage that measures
on the label map is one entry of _STAGES (_MAP_STAGES: those that measure it against maps the caller brings), and one _Layout per
batch owns every offset into the batch's two shared buffers.
DESIGN.md section 13 describes both.
"""
from __future__ import annotations

import collections
import dataclasses
from typing import NamedTuple

import numpy as np
import torch
from utils import droplet_cells, droplet_confidence, droplet_hull, droplet_neighbors, droplet_shape

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
    labels: also the int32 label map; needs a split depth or a stage that reads the label map (label_map).
    thresh_low (<= thresh) / max_hole_area (0 = off, negative = any size, N = holes of at most N pixels): the mask is
    cleaned first (hysteresis threshold, hole filling: csrc/clean.hip).
    neighbors (contact radius in pixels, an integer 1..64; None = off): also the contact pairs and the per-droplet nearest
    contact, degree and cluster (csrc/neighbors.hip, utils/droplet_neighbors.py).
    confidence (the uncertainty band, 0..0.5; None = off): also the per-droplet and per-image integers of the quantised
    probability, its entropy and, given envelope=(lo, hi), the disagreement of the TTA variants (csrc/confidence.hip,
    utils/droplet_confidence.py); confidence_maps: also the uint8 entropy and spread maps, on the device.
    hull: also the per-droplet integers of the convex hull that utils.droplet_hull.hull_columns reads (csrc/hull.hip, DESIGN.md
    section 24).
    cells: also the per-droplet and per-cell integers of utils.droplet_cells.cells_record against the cell label maps given as
    the keyword cells= (one cells.CellMap per image; csrc/cells.hip).
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
    cells: bool = False
    thresh: dataclasses.InitVar[float | None] = None
    gray: dataclasses.InitVar[object] = None

    def __post_init__(self, thresh, gray):
        if self.labels and self.split_depth is None and not self.label_map:
            raise _lib.UnetdcError("return_labels needs a split_depth or a stage on the label map: " + ", ".join(S.option for S in _STAGES + _MAP_STAGES))
        try:
            if self.neighbors is not None:
                droplet_neighbors.check_radius(self.neighbors)
            if self.confidence is not None:
                droplet_confidence.check_band(self.confidence)
        except ValueError as e:
            raise _lib.UnetdcError(str(e)) from None
        if self.confidence_maps and self.confidence is None:
            raise _lib.UnetdcError("confidence_maps needs confidence (the band)")
        if gray is not None and not self.shape:
            raise _lib.UnetdcError("gray needs shape=True")
        if thresh is not None:
            self.cleaning(thresh)

    @property
    def label_map(self):
        """Whether a stage of _STAGES reads the int32 label map (without a split depth that selects unetdc_ccl_labels)."""
        return any(S.on(self) for S in _STAGES + _MAP_STAGES)

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
    gray; envelope; the cell maps).  options=DropletOptions(...), or its fields by name (labels also under its earlier name
    return_labels; cells= carries the maps themselves and switches the field on)."""
    kw = dict(keywords)
    gray, base, envelope = kw.pop("gray", None), kw.pop("options", None) or DropletOptions(), kw.pop("envelope", None)
    cells = kw.pop("cells", None)
    if cells is not None:
        kw["cells"] = True
    if "return_labels" in kw:
        kw["labels"] = kw.pop("return_labels")
    opts = dataclasses.replace(base, **kw, thresh=thresh, gray=gray)
    if envelope is not None and opts.confidence is None:
        raise _lib.UnetdcError("envelope needs confidence (the band)")
    if opts.cells and cells is None:
        raise _lib.UnetdcError("cells=True needs the cell maps: cells=[cells.CellMap(label, max_label, d2), ...], one per image")
    return opts, gray, envelope, cells


@dataclasses.dataclass(eq=False)
class Droplets:
    """One image's result.  Iterates as (mask, area, centroid_row, centroid_col); the rest is reached by name.
    mask: uint8 [oh, ow] DEVICE tensor; area int64 [n], centroid_row / centroid_col float64 [n]: droplets in the
    reference's label order; labels: int32 [oh, ow] DEVICE label map (None unless asked for); props: the dict of
    per-droplet int64 arrays that utils.droplet_shape.shape_columns reads (None without shape); clean_counts: int64 [4],
    the counts of utils.droplet_clean.COUNT_NAMES (zeros when cleaning is off); neighbors: the record of
    utils.droplet_neighbors.neighbors_numpy, int64 arrays (None unless asked for); confidence: the record of
    utils.droplet_confidence.confidence_numpy (None unless asked for), its two maps DEVICE tensors; hull: the dict of five int64
    arrays that utils.droplet_hull.hull_columns reads (None unless asked for); cells: the record of
    utils.droplet_cells.cells_record (None unless asked for).  The CPU path of the script fills the same record
    with host arrays."""
    mask: object
    area: np.ndarray
    centroid_row: np.ndarray
    centroid_col: np.ndarray
    labels: object = None
    props: dict | None = None
    clean_counts: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(4, np.int64))
    neighbors: dict | None = None
    confidence: dict | None = None
    hull: dict | None = None
    cells = None      # the record of a _MAP_STAGES stage: a plain attribute that with_records sets, not one more constructor argument

    def __iter__(self):
        return iter((self.mask, self.area, self.centroid_row, self.centroid_col))

    def with_records(self, **records):
        """Sets the records of the stages that are not fields (cells) -> self."""
        for name, rec in records.items():
            if not hasattr(type(self), name):
                raise AttributeError(name)
            setattr(self, name, rec)
        return self


class _Image(NamedTuple):
    """One image's views into the batch's buffers."""
    probs: torch.Tensor           # fp32 [ph, pw]
    mask: torch.Tensor            # uint8 [oh, ow]
    label: torch.Tensor | None    # int32 [oh, ow]
    gray: torch.Tensor | None     # uint8 [oh, ow]
    count: torch.Tensor           # int32, the droplet count first
    area: torch.Tensor            # int32 [cap]
    sums: torch.Tensor            # int64 [layout.n_rows, cap]: sum y, sum x, then the rows of the stages
    clean_counts: torch.Tensor | None   # int32, the four counts
    stage: dict                   # by the field of each stage that is on: its views of this image (_Stage.views and _droplets)


# What the launches of one batch share.  ws: the one workspace, uint8, used in stream order; cap: the droplets per image that the
# outputs hold; rooms: by _Stage.room, the slots per image of each growable room; envelope: (lo, hi) fp32 [B, ph, pw] or None;
# cells: B cells.CellMap or None.
_Batch = collections.namedtuple("_Batch", "opts thresh min_area stream ws cap rooms layout counts envelope cells")


class _Layout:
    """Where everything lies in the two buffers that a batch shares, computed once from (B, the stages that are on, whether
    the mask is cleaned); the launches and the readback both index through it.
    counts, int32, zeroed: B droplet counts, 4 clean counts per image, then each stage's slots32 per image in stage order;
    from `tail`, the next even index (an 8-byte boundary), as int64: each stage's slots64 per image.
    sums, int64 [n_rows, B, cap]: sum y, sum x, then each stage's rows, in one piece as its kernel wants them."""

    def __init__(self, B, stages, clean):
        self.B, self.at32, self.at64, self.at_row, n, m, r = B, {}, {}, {}, 0, 0, 2
        for name, per in [("count", 1), ("clean", 4 * bool(clean))] + [(S.field, S.slots32) for S in stages]:
            self.at32[name], n = (n, per), n + per * B
        for S in stages:
            self.at64[S.field], m = (m, S.slots64), m + S.slots64 * B
            self.at_row[S.field], r = (r, S.rows), r + S.rows
        self.n32, self.tail, self.n_rows = n, (n + 1) // 2 * 2, r
        self.n_counts = self.tail + 2 * m if m else n

    def int32(self, counts, name, i=None):
        """The int32 slots of `name` in counts (device or host): image i's, or the whole batch's."""
        at, per = self.at32[name]
        return counts[at:at + per * self.B] if i is None else counts[at + per * i:at + per * (i + 1)]

    def int64(self, counts, name, i):
        """Image i's int64 slots of the stage `name` in the tail of counts (device or host)."""
        at, per = self.at64[name]
        return counts[self.tail:].view(torch.int64 if torch.is_tensor(counts) else np.int64)[at + per * i:at + per * (i + 1)]

    def rows(self, sums, name):
        """The rows of the stage `name` in one image's sums [n_rows, ...] (device or host)."""
        at, k = self.at_row[name]
        return sums[at:at + k]

    def views(self, counts, sums, S, i):
        """Image i's part of the stage S on the device, by name: "rows" of its sums, "needed" (slots32) and "totals" (slots64)."""
        v = {"rows": self.rows(sums, S.field)} if S.rows else {}
        if S.slots32:
            v["needed"] = self.int32(counts, S.field, i)
        if S.slots64:
            v["totals"] = self.int64(counts, S.field, i)
        return v


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Stage:
    """An optional stage that measures on the label map: what it needs of the batch's buffers, its launch(b, im, v) behind
    the labelling (v: im.stage[field], with "needed" = its slots32, "totals" = its slots64 and "rows" = its rows of im.sums)
    and record(b, i, im, area, sums, raw) from the host copies.  One instance per batch; _STAGES below holds the subclasses
    in launch order, and nothing else names a stage."""
    option = field = None         # the DropletOptions field that switches it on (None / False: off), the Droplets field it fills
    slots32 = slots64 = rows = 0  # per image: int32 slots in counts, int64 slots in its tail; per droplet: int64 rows in sums
    room = None                   # the name of its growable room; slots32[0] is then what the image needed of it, and
    #                               capacity(cap, out_hws, wanted) -> the slots it gets, limit(hw) -> (the most there can be, the error)
    workspace = staticmethod(lambda lib, h, w, cap, rooms: 0)

    def __init__(self, b):
        pass

    @classmethod
    def on(cls, opts):
        v = getattr(opts, cls.option)
        return v is not None and v is not False

    def views(self, b, i, hw):
        """Image i's device tensors beyond those of the layout, by name."""
        return {}

    def fetch(self, b, ints, nmax):
        """Further device->host copies, once the counts are on the host (ints: their int32 part as int64)."""


class _Props(_Stage):
    """csrc/shape.hip: the integers utils.droplet_shape.shape_columns reads, under the names of label_props_numpy."""
    option, field, rows = "shape", "props", len(droplet_shape.QUANTITIES)

    def launch(self, b, im, v):
        _lib.call("unetdc_label_props", im.label.data_ptr(), _ptr(im.gray), *im.mask.shape, v["rows"][0].data_ptr(), b.cap, b.stream)

    def record(self, b, i, im, area, sums, raw):
        rows = zip(droplet_shape.QUANTITIES, b.layout.rows(sums, self.field))
        return {"area": area, "Sy": sums[0], "Sx": sums[1],
                **{q: r for q, r in rows if im.gray is not None or q not in droplet_shape.GRAY_QUANTITIES}}


PAIR_ROOM = 1 << 14    # contact pairs per image the first launch has room for; an image with more is run again with twice that
MAX_PAIR_ROOM = 1 << 27   # the largest table of unetdc_label_neighbors


class _Neighbors(_Stage):
    """csrc/neighbors.hip: the record of utils.droplet_neighbors.neighbors_numpy; the capacity is the kernel's max_label.  Its
    integers are int32 planes of its own, [3, pair room] (a, b, d2) and [5, cap] (COLUMN_NAMES) per image: two more copies."""
    option, field, slots32, room = "neighbors", "neighbors", 1, "pairs"
    # cap labels have at most cap (cap - 1) / 2 pairs
    capacity = staticmethod(lambda cap, out_hws, wanted: int(min(PAIR_ROOM if wanted is None else wanted, cap * (cap - 1) // 2, MAX_PAIR_ROOM)))
    limit = staticmethod(lambda hw: (MAX_PAIR_ROOM, f"more than {MAX_PAIR_ROOM} contact pairs in one image"))
    workspace = staticmethod(lambda lib, h, w, cap, rooms: lib.unetdc_label_neighbors_workspace(h, w, cap, rooms["pairs"]))

    def __init__(self, b):
        self.pairs = torch.empty(b.layout.B, 3, b.rooms["pairs"], dtype=torch.int32, device=b.counts.device)
        self.per_label = torch.empty(b.layout.B, 5, b.cap, dtype=torch.int32, device=b.counts.device)

    def views(self, b, i, hw):
        return {"pairs": self.pairs[i], "per_label": self.per_label[i]}

    def launch(self, b, im, v):
        room = b.rooms["pairs"]
        _lib.call("unetdc_label_neighbors", im.label.data_ptr(), b.cap, *im.mask.shape, int(b.opts.neighbors), b.ws.data_ptr(), b.ws.numel(),
                  v["needed"].data_ptr(), *((v["pairs"][j].data_ptr() if room else None) for j in range(3)), room,
                  *(v["per_label"][j].data_ptr() for j in range(5)), b.stream)

    def fetch(self, b, ints, nmax):
        self.n_pairs = b.layout.int32(ints, self.field)
        self.per_label_h = self.per_label[:, :, :nmax].cpu().numpy().astype(np.int64)
        self.pairs_h = self.pairs[:, :, :int(min(self.n_pairs.max(initial=0), b.rooms["pairs"]))].cpu().numpy().astype(np.int64)

    def record(self, b, i, im, area, sums, raw):
        return {"pairs": dict(zip(("a", "b", "d2"), self.pairs_h[i, :, :self.n_pairs[i]])),
                **dict(zip(droplet_neighbors.COLUMN_NAMES, self.per_label_h[i, :, :len(area)]))}


_tables = {}


def _entropy_table(device):
    """utils.droplet_confidence.entropy_table on the device, uploaded once per device (128 KB; int16 holds the uint16 bits)."""
    key = str(device)
    if key not in _tables:
        _tables[key] = torch.from_numpy(droplet_confidence.entropy_table().view(np.int16).copy()).to(device)
    return _tables[key]


class _Confidence(_Stage):
    """csrc/confidence.hip: the record of utils.droplet_confidence.confidence_numpy; the capacity is the kernel's max_out.  Its
    slots64 are the per-image totals (IMAGE_QUANTITIES); its two uint8 maps stay on the device."""
    option, field = "confidence", "confidence"
    slots64, rows = len(droplet_confidence.IMAGE_QUANTITIES), len(droplet_confidence.CONF_QUANTITIES)

    def views(self, b, i, hw):
        lo, hi = (None, None) if b.envelope is None else (t[i] for t in b.envelope)
        maps = [torch.empty(hw, dtype=torch.uint8, device=b.counts.device) if b.opts.confidence_maps and read else None
                for read in (True, lo is not None)]               # the spread map only with an envelope
        return {"lo": lo, "hi": hi, "entropy_u8": maps[0], "spread_u8": maps[1]}

    def launch(self, b, im, v):
        _lib.call("unetdc_label_confidence", im.label.data_ptr(), b.cap, *im.mask.shape, im.probs.data_ptr(), _ptr(v["lo"]), _ptr(v["hi"]),
                  *im.probs.shape, float(b.thresh), float(b.opts.confidence), _entropy_table(im.probs.device).data_ptr(),
                  v["rows"][0].data_ptr(), v["totals"].data_ptr(), _ptr(v["entropy_u8"]), _ptr(v["spread_u8"]), b.stream)

    def record(self, b, i, im, area, sums, raw):
        v = im.stage[self.field]
        return {**dict(zip(droplet_confidence.CONF_QUANTITIES, b.layout.rows(sums, self.field))), "image": b.layout.int64(raw, self.field, i),
                "envelope": b.envelope is not None, "entropy_u8": v["entropy_u8"], "spread_u8": v["spread_u8"]}


# Row-extent slots per droplet of the capacity that the first launch of unetdc_label_hull has room for.  The slots needed are the
# sum of the droplets' heights.  The droplets of the flow are connected, so that sum is at most h * w, and the room is capped
# there: then it always suffices.  Below the cap, 64 rows per droplet is three times the about 20 rows of a median droplet of a
# 1040 x 1388 micrograph and 512 KB of workspace per 1024 droplets; an image of taller droplets than that is run again with
# twice the room, like one with more contact pairs than the pair lists hold.
ROWS_PER_DROPLET = 64


class _Hull(_Stage):
    """csrc/hull.hip: the integers utils.droplet_hull.hull_columns reads; the capacity is the kernel's max_out."""
    option, field, slots32, room, rows = "hull", "hull", 1, "rows", len(droplet_hull.QUANTITIES)
    capacity = staticmethod(lambda cap, out_hws, wanted: int(min(ROWS_PER_DROPLET * cap if wanted is None else wanted, max(h * w for h, w in out_hws))))
    limit = staticmethod(lambda hw: (hw[0] * hw[1], "unetdc_label_hull: connected droplets need more row room than the image has pixels"))
    workspace = staticmethod(lambda lib, h, w, cap, rooms: lib.unetdc_label_hull_workspace(h, w, cap, rooms["rows"]))

    def launch(self, b, im, v):
        _lib.call("unetdc_label_hull", im.label.data_ptr(), b.cap, *im.mask.shape, b.ws.data_ptr(), b.ws.numel(), v["rows"][0].data_ptr(),
                  v["needed"].data_ptr(), b.rooms["rows"], b.stream)

    def record(self, b, i, im, area, sums, raw):
        return dict(zip(droplet_hull.QUANTITIES, b.layout.rows(sums, self.field)))


TRIPLE_ROOM = 1 << 14    # (droplet, cell) pairs per image the first launch has room for; an image with more is run again with twice that


class _Cells(_Stage):
    """csrc/cells.hip: the record of utils.droplet_cells.cells_record against the image's cells.CellMap; the capacity is the
    kernel's max_droplet.  Its integers are planes of its own: int32 [6, cap] per image and int64 [8, max_cell] per image, the
    latter with the image's own max_cell as the row length, in a buffer sized for the largest: two more copies."""
    option, field, slots32, room = "cells", "cells", 1, "triples"
    # a pixel carries at most one pair: h * w always suffices
    capacity = staticmethod(lambda cap, out_hws, wanted: int(min(TRIPLE_ROOM if wanted is None else wanted, max(h * w for h, w in out_hws))))
    limit = staticmethod(lambda hw: (hw[0] * hw[1], "unetdc_cell_table: more (droplet, cell) pairs than the image has pixels"))
    # max_cell has no plane in the workspace (the per-cell sums go straight to the output): the query does not read it
    workspace = staticmethod(lambda lib, h, w, cap, rooms: lib.unetdc_cell_table_workspace(h, w, cap, 0, rooms["triples"]))
    ND, NC = len(droplet_cells.DROPLET_QUANTITIES), len(droplet_cells.CELL_QUANTITIES)

    def __init__(self, b):
        dev = b.counts.device
        self.per_droplet = torch.empty(b.layout.B, self.ND, b.cap, dtype=torch.int32, device=dev)
        self.per_cell = torch.empty(b.layout.B, self.NC * max(c.max_label for c in b.cells), dtype=torch.int64, device=dev)

    def views(self, b, i, hw):
        m = b.cells[i]
        return {"map": m, "per_droplet": self.per_droplet[i], "per_cell": self.per_cell[i, :self.NC * m.max_label].view(self.NC, m.max_label)}

    def launch(self, b, im, v):
        m = v["map"]
        _lib.call("unetdc_cell_table", im.label.data_ptr(), b.cap, m.label.data_ptr(), m.max_label, _ptr(m.d2), *im.mask.shape,
                  b.ws.data_ptr(), b.ws.numel(), v["needed"].data_ptr(), b.rooms["triples"], v["per_droplet"].data_ptr(),
                  v["per_cell"].data_ptr() if m.max_label else None, b.stream)

    def fetch(self, b, ints, nmax):
        self.per_droplet_h = self.per_droplet[:, :, :nmax].cpu().numpy().astype(np.int64)
        self.per_cell_h = self.per_cell.cpu().numpy()       # sized by the largest label: a caller with sparse ids renumbers them first

    def record(self, b, i, im, area, sums, raw):
        m = b.cells[i]
        return droplet_cells.make_record(self.per_droplet_h[i, :, :len(area)],
                                         self.per_cell_h[i, :self.NC * m.max_label].reshape(self.NC, m.max_label), m.d2 is not None)


_STAGES = (_Props, _Neighbors, _Confidence, _Hull)     # in launch order, which is the order of their slots and rows
# behind them, the stages that measure the label map against maps the caller brings (the keyword of their field): their slots
# and rows lie behind those of _STAGES, so a batch without them keeps the layout it had
_MAP_STAGES = (_Cells,)


def _enqueue(im, b, stages):
    """One image's launches on the batch's stream: the mask of the threshold; unetdc_mask_clean in place on it (the weak
    mask is that of the low threshold under the same resize rule); labelling + sums + compaction by unetdc_ccl_stats,
    with a split depth unetdc_split_stats (which also fills the label map when there is one), with a stage and no split
    depth unetdc_ccl_labels; then every stage that is on, on the label map, the droplet capacity as its max_label / max_out."""
    (oh, ow), opts, ws, s = im.mask.shape, b.opts, b.ws, b.stream
    h2, clean = opts.half_pixels, opts.cleaning(b.thresh)
    _mask_from_probs(im.probs, b.thresh, im.mask, s)
    if clean is not None:
        low, holes = clean
        weak = None
        if low is not None:
            weak = torch.empty_like(im.mask)
            _mask_from_probs(im.probs, low, weak, s)
        _lib.call("unetdc_mask_clean", im.mask.data_ptr(), _ptr(weak), oh, ow, holes, ws.data_ptr(), ws.numel(), im.mask.data_ptr(),
                  im.clean_counts.data_ptr(), s)
    head = (im.mask.data_ptr(), oh, ow, int(max(b.min_area, 1)))
    outs = (ws.data_ptr(), ws.numel(), im.count.data_ptr(), im.area.data_ptr(), im.sums[0].data_ptr(), im.sums[1].data_ptr(), None)
    if h2 is not None:
        _lib.call("unetdc_split_stats", *head, h2, *outs, _ptr(im.label), b.cap, s)
    elif stages:
        _lib.call("unetdc_ccl_labels", *head, *outs, _ptr(im.label), b.cap, s)
    else:
        _lib.call("unetdc_ccl_stats", *head, *outs, b.cap, s)
    for st in stages:
        st.launch(b, im, im.stage[st.field])


def _workspace_bytes(lib, out_hws, opts, clean, stages, cap, rooms):
    """The one workspace holds the largest need of any launch of any image."""
    head = (lib.unetdc_split_workspace if opts.split_depth is not None else
            lib.unetdc_ccl_labels_workspace if opts.label_map else lib.unetdc_ccl_workspace)
    return max(max(head(h, w), lib.unetdc_mask_clean_workspace(h, w) if clean is not None else 0,
                   *(S.workspace(lib, h, w, cap, rooms) for S in stages)) for h, w in out_hws)


def _droplets(probs, thresh, out_hws, min_area, wanted, gray, opts, envelope=None, cells=None):
    """The one launch-and-readback body -> (B Droplets, the device outputs (count, area, sumy, sumx) or None when an image
    had more droplets than they hold).  wanted: the rooms asked for by name, "droplets" (the capacity) and optionally those of
    the stages (_Stage.room; their defaults otherwise).  Every launch of the batch is enqueued back to back on the current
    stream into ONE int32 and ONE int64 buffer (_Layout); the host then waits ONCE: one device->host copy brings every count
    and per-image total, two more the filled part of the per-droplet integers, and a stage may add copies of planes of its
    own (_Stage.fetch).  An image that needed more of a room than there was is run again alone with that room enlarged:
    droplets to the exact count, a stage's to twice what it had, up to the stage's limit."""
    if not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 3:
        raise _lib.UnetdcError("mask_and_droplets_batch needs a [B, H, W] fp32 tensor on the HIP device")
    probs = probs.contiguous()
    if envelope is not None:
        if len(envelope) != 2 or any(not torch.is_tensor(t) or t.dtype != torch.float32 or t.shape != probs.shape or t.device != probs.device
                                     for t in envelope):
            raise _lib.UnetdcError("envelope is (lo, hi): two fp32 tensors shaped like probs, on its device")
        envelope = tuple(t.contiguous() for t in envelope)
    B, dev, clean = probs.shape[0], probs.device, opts.cleaning(thresh)
    out_hws = [(int(h), int(w)) for h, w in out_hws]
    cap = int(min(wanted["droplets"], max(h * w for h, w in out_hws)))
    for g, hw in zip(() if gray is None else gray, out_hws):
        if not g.is_cuda or g.dtype != torch.uint8 or tuple(g.shape) != hw or not g.is_contiguous():
            raise _lib.UnetdcError("gray must be a contiguous uint8 [oh, ow] tensor on the HIP device")
    if opts.cells:
        if len(cells) != B:
            raise _lib.UnetdcError("cells: one cells.CellMap per image")
        for m, hw in zip(cells, out_hws):
            for t in (m.label,) + (() if m.d2 is None else (m.d2,)):
                if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != hw or not t.is_contiguous():
                    raise _lib.UnetdcError("cells: label and d2 must be contiguous int32 [oh, ow] tensors on the HIP device")
            if int(m.max_label) < 0:
                raise _lib.UnetdcError("cells: max_label must not be negative")
    on = [S for S in _STAGES + _MAP_STAGES if S.on(opts)]
    rooms = {S.room: S.capacity(cap, out_hws, wanted.get(S.room)) for S in on if S.room}
    lay = _Layout(B, on, clean is not None)
    ws = torch.empty(_workspace_bytes(_lib.load(), out_hws, opts, clean, on, cap, rooms), dtype=torch.uint8, device=dev)   # one: stream order
    counts = torch.zeros(lay.n_counts, dtype=torch.int32, device=dev)
    area = torch.empty(B, cap, dtype=torch.int32, device=dev)
    sums = torch.empty(B, lay.n_rows, cap, dtype=torch.int64, device=dev).permute(1, 0, 2)
    b = _Batch(opts, thresh, min_area, torch.cuda.current_stream().cuda_stream, ws, cap, rooms, lay, counts, envelope, cells if opts.cells else None)
    stages, images = [S(b) for S in on], []
    for i, hw in enumerate(out_hws):
        view = sums[:, i]
        images.append(_Image(probs=probs[i], mask=torch.empty(hw, dtype=torch.uint8, device=dev),
                             label=torch.empty(hw, dtype=torch.int32, device=dev) if opts.labels or on else None,
                             gray=None if gray is None else gray[i], count=lay.int32(counts, "count", i), area=area[i], sums=view,
                             clean_counts=None if clean is None else lay.int32(counts, "clean", i),
                             stage={st.field: {**st.views(b, i, hw), **lay.views(counts, view, st, i)} for st in stages}))
        _enqueue(images[i], b, stages)
    raw = counts.cpu().numpy()                                      # the batch's only host wait
    ints = raw[:lay.n32].astype(np.int64)
    n = lay.int32(ints, "count")
    clean_counts = lay.int32(ints, "clean").reshape(B, 4) if clean is not None else np.zeros((B, 4), np.int64)
    nmax = int(min(n.max(initial=0), cap))
    a_h = area[:, :nmax].cpu().numpy().astype(np.int64)
    s_h = sums[:, :, :nmax].cpu().numpy()
    for st in stages:
        st.fetch(b, ints, nmax)

    def overflowed(i):
        """The room that image i needed more of than there was, enlarged (droplets first, then the stages' in their order)."""
        if n[i] > cap:
            return {"droplets": int(n[i])}
        for st in stages:
            if st.room and lay.int32(ints, st.field, i)[0] > rooms[st.room]:
                most, error = st.limit(out_hws[i])
                if rooms[st.room] >= most:
                    raise _lib.UnetdcError(error)
                return {st.room: 2 * max(rooms[st.room], 1)}

    out = []
    for i, im in enumerate(images):
        more = overflowed(i)
        if more:                                  # this image again, alone
            out.append(_droplets(probs[i:i + 1], thresh, out_hws[i:i + 1], min_area, {**wanted, **more}, None if gray is None else gray[i:i + 1],
                                 opts, None if envelope is None else tuple(t[i:i + 1] for t in envelope),
                                 None if cells is None else cells[i:i + 1])[0][0])
            continue
        a, si = a_h[i, :n[i]], s_h[:, i, :n[i]]
        d = np.maximum(a, 1)
        recs = {st.field: (st.record(b, i, im, a, si, raw), type(st) in _STAGES) for st in stages}
        out.append(Droplets(im.mask, a, si[0].astype(np.float64) / d, si[1].astype(np.float64) / d, labels=im.label if opts.labels else None,
                            clean_counts=clean_counts[i], **{f: r for f, (r, field) in recs.items() if field})
                   .with_records(**{f: r for f, (r, field) in recs.items() if not field}))
    return out, ((lay.int32(counts, "count"), area, sums[0], sums[1]) if n.max(initial=0) <= cap else None)


def mask_and_droplets_batch(probs, thresh, out_hws, min_area, max_droplets=1 << 14, keep_sums=False, **options):
    """probs: [B, H, W] fp32 probabilities on the HIP device; out_hws: B (oh, ow) pairs -> a list of B Droplets, after
    ONE host wait for the whole batch (_droplets).  keep_sums=True returns (that list, the device outputs (count, area,
    sumy, sumx) or None when an image had more droplets than they hold) for density.density_maps_batch.
    options: split_depth, shape, return_labels, thresh_low, max_hole_area, neighbors, confidence, confidence_maps, hull by name, or
    options=DropletOptions(...); gray=B uint8 [oh, ow] DEVICE tensors for the intensity integers of shape (None: none);
    envelope=(lo, hi), two fp32 DEVICE tensors shaped like probs (tta.predict_tta(..., envelope=True)), for the disagreement
    integers of confidence (None: those keep their initial values); and cells=B cells.CellMap (the cell label map of each image,
    its largest label and optionally the d2 plane of cells.nearest_label) for the per-cell table.  Every option adds its launches
    behind each image's existing ones and its integers to the copies the host already waits for; all off: no launch is added."""
    opts, gray, envelope, cells = _options(options, thresh)
    out, sums = _droplets(probs, thresh, out_hws, min_area, {"droplets": max_droplets}, gray, opts, envelope, cells)
    return (out, sums) if keep_sums else out


def mask_and_droplets(probs2d, thresh, out_hw, min_area, max_droplets=1 << 16, **options):
    """probs2d: [H, W] fp32 probabilities on the HIP device -> its Droplets: the batch of one.  options as in
    mask_and_droplets_batch; gray: one uint8 [oh, ow] DEVICE tensor; envelope: two fp32 [H, W] DEVICE tensors; cells: one
    cells.CellMap."""
    opts, gray, envelope, cells = _options(options, thresh)
    return _droplets(probs2d[None], thresh, [out_hw], min_area, {"droplets": max_droplets}, None if gray is None else [gray], opts,
                     None if envelope is None else tuple(t[None] for t in envelope), None if cells is None else [cells])[0][0]

