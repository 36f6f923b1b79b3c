"""Difference map of a predicted mask against an annotated one, and its 8-connected regions.

The host path of what ``unetdc_diff_regions`` and ``unetdc_diff_paint`` compute on the device (csrc/diffmap.hip), and the
table code both paths share.  Integer work only: the two paths agree bit for bit.

Class plane ``c = pred | gt << 1`` (nonzero counts as 1) and the reference's colours (train_DC_focal.py:create_difference_map):

    0 black  (0, 0, 0)      neither            TN
    1 green  (0, 255, 0)    only predicted     FP
    2 red    (255, 0, 0)    only annotated     FN
    3 yellow (255, 255, 0)  both               TP

A region is a maximal 8-connected set of pixels of equal class; all four classes count, black included (the reference's
count_color_regions_in_memory).  The record of an image:

    image      int64 [12]: pixels[4], regions[4] (every region), kept[4] (regions of at least min_area pixels), by class
    class, area, sumy, sumx, neighbors   int64 arrays, one entry per region of class 1..3 with area >= min_area, in raster
               order of the region's first pixel; bit k of neighbors: some pixel of the region has an 8-neighbour of class
               k != class (the image border sets no bit)
"""
from __future__ import annotations

import numpy as np

COLORS = np.array([(0, 0, 0), (0, 255, 0), (255, 0, 0), (255, 255, 0)], dtype=np.uint8)
CLASS_NAMES = ("black", "green", "red", "yellow")
BLACK, GREEN, RED, YELLOW = 0, 1, 2, 3
TABLE_KEYS = ("class", "area", "sumy", "sumx", "neighbors")
COUNT_COLUMNS = tuple(f"{CLASS_NAMES[c]}_blobs" for c in (YELLOW, RED, GREEN, BLACK))


def class_plane(pred, gt):
    """uint8 [h, w]: (pred != 0) | (gt != 0) << 1."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.ndim != 2 or pred.shape != gt.shape:
        raise ValueError(f"prediction {pred.shape} and annotation {gt.shape} must be two planes of one size")
    return (pred != 0).astype(np.uint8) | ((gt != 0).astype(np.uint8) << 1)


def difference_map_rgb(pred, gt):
    """uint8 [h, w, 3]: the colour of the class plane (the reference's create_difference_map(gt, pred))."""
    return COLORS[class_plane(pred, gt)]


def overlay_difference(image, pred, gt):
    """uint8 [h, w, 3]: `image` (HWC uint8 RGB) with every pixel of class != 0 replaced by its colour."""
    image = np.asarray(image)
    c = class_plane(pred, gt)
    if image.dtype != np.uint8 or image.shape != c.shape + (3,):
        raise ValueError(f"the image must be uint8 {c.shape + (3,)}, not {image.dtype} {image.shape}")
    out = image.copy()
    out[c != 0] = COLORS[c[c != 0]]
    return out


def _shifted(c, dy, dx, fill):
    """c moved so that entry (y, x) holds c[y + dy, x + dx], `fill` where that lies outside."""
    h, w = c.shape
    out = np.full_like(c, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = c[ys, xs]
    return out


def neighbor_bits(c):
    """int64 [h, w]: per pixel the OR of 1 << class over its 8 neighbours inside the image, its own class bit cleared."""
    bits = np.zeros(c.shape, np.int64)
    one = np.int64(1)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                s = _shifted(c, dy, dx, 255)
                bits |= np.where(s != 255, one << np.minimum(s, 3).astype(np.int64), 0)
    return bits & ~(one << c.astype(np.int64))


def diff_regions_numpy(pred, gt, min_area=1):
    """The record of the module docstring from two host planes (scipy.ndimage.label with the full 3 x 3 structure per class)."""
    from scipy import ndimage
    if int(min_area) < 1:
        raise ValueError("min_area is at least 1")
    c = class_plane(pred, gt)
    h, w = c.shape
    index = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ys, xs = np.divmod(index, w)
    bits = neighbor_bits(c)
    image = np.zeros(12, np.int64)
    rows = {k: [] for k in TABLE_KEYS}
    first = []
    for k in range(4):
        lab, n = ndimage.label(c == k, structure=np.ones((3, 3), int))
        image[k] = int((c == k).sum())
        image[4 + k] = n
        if n == 0:
            continue
        flat = lab.ravel()
        area = np.bincount(flat, minlength=n + 1)[1:]
        keep = area >= int(min_area)
        image[8 + k] = int(keep.sum())
        if k == BLACK or not keep.any():
            continue
        ids = np.arange(1, n + 1)
        nb = np.zeros(n + 1, np.int64)
        for b in range(4):
            nb[np.unique(flat[(bits.ravel() >> b) & 1 == 1])] |= 1 << b
        first.append(np.asarray(ndimage.minimum(index, lab, ids), np.int64)[keep])
        rows["class"].append(np.full(int(keep.sum()), k, np.int64))
        rows["area"].append(area[keep].astype(np.int64))
        rows["sumy"].append(_label_sum(flat, ys.ravel(), n)[keep])
        rows["sumx"].append(_label_sum(flat, xs.ravel(), n)[keep])
        rows["neighbors"].append(nb[1:][keep])
    rec = {"image": image}
    if first:
        order = np.argsort(np.concatenate(first), kind="stable")
        for k in TABLE_KEYS:
            rec[k] = np.concatenate(rows[k]).astype(np.int64)[order]
    else:
        for k in TABLE_KEYS:
            rec[k] = np.zeros(0, np.int64)
    return rec


def _label_sum(flat, values, n):
    """int64 [n]: the sum of the coordinates `values` over the pixels of labels 1..n.  Every partial sum is an integer below
    2^30 * 2^14 < 2^53, so the float64 accumulator of bincount is exact."""
    return np.bincount(flat, weights=values.astype(np.float64), minlength=n + 1)[1:].astype(np.int64)


def touches(rec, k):
    """bool per table row: the region borders class k."""
    return (rec["neighbors"] >> k) & 1 == 1


def region_table(filename, rec, px_per_um=None):
    """The rows of diff_regions.csv for one image: filename, class (green / red / yellow), area, centroid-0, centroid-1,
    touches_common (a yellow neighbour; False on yellow regions), isolated (a red or green region without one: a droplet
    missed entirely, or a spurious one), and with px_per_um area_sqmicron."""
    n = len(rec["class"])
    area = rec["area"].astype(np.float64)
    common = touches(rec, YELLOW)
    cols = {"filename": [filename] * n, "class": [CLASS_NAMES[int(k)] for k in rec["class"]], "area": rec["area"],
            "centroid-0": rec["sumy"] / np.maximum(area, 1.0), "centroid-1": rec["sumx"] / np.maximum(area, 1.0),
            "touches_common": common, "isolated": (rec["class"] != YELLOW) & ~common}
    if px_per_um is not None:
        cols["area_sqmicron"] = area / (px_per_um ** 2)
    return cols


IMAGE_COLUMNS = (COUNT_COLUMNS + tuple(f"{CLASS_NAMES[c]}_px" for c in (YELLOW, RED, GREEN, BLACK)) +
                 tuple(f"{CLASS_NAMES[c]}_kept" for c in (YELLOW, RED, GREEN, BLACK)) + ("missed_droplets", "spurious_droplets"))


def image_columns(rec):
    """The integers of one row of diff_regions_per_image.csv: the reference's four region counts (yellow_blobs = region-level
    TP, red_blobs FN, green_blobs FP, black_blobs TN), the pixel counts, the regions of at least min_area pixels, and among
    those missed_droplets (red without a yellow neighbour) and spurious_droplets (green without one)."""
    im = rec["image"]
    lone = ~touches(rec, YELLOW)
    out = {}
    for c in (YELLOW, RED, GREEN, BLACK):
        out[f"{CLASS_NAMES[c]}_blobs"] = int(im[4 + c])
    for c in (YELLOW, RED, GREEN, BLACK):
        out[f"{CLASS_NAMES[c]}_px"] = int(im[c])
    for c in (YELLOW, RED, GREEN, BLACK):
        out[f"{CLASS_NAMES[c]}_kept"] = int(im[8 + c])
    out["missed_droplets"] = int(((rec["class"] == RED) & lone).sum())
    out["spurious_droplets"] = int(((rec["class"] == GREEN) & lone).sum())
    return out


def sum_image_columns(rows):
    """Column-wise sum of image_columns() dicts (all zeros for none)."""
    return {k: int(sum(r[k] for r in rows)) for k in IMAGE_COLUMNS}
