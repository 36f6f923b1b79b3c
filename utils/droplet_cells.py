"""Droplets per cell on the CPU: the nearest-label transform and the per-cell table that
csrc/cells.hip computes on the device, in numpy, with the same integers bit for bit; the column formulas of the script
(per-droplet columns, cells.csv, the per-image summary) and the checks of its flags.

Definitions (include/unetdc_hip.h holds the same text).  Seed pixels are the pixels q with 1 <= label[q] <= max_label.  For
every pixel p, (d2[p], L) is the lexicographic minimum over the seed pixels of (|p - q|^2, label[q]): the nearest seed pixel
wins, among equidistant ones the smallest label.  A radius > 0 zeroes the label where d2 > radius^2; d2 stays exact.
"""
from __future__ import annotations

import math

import numpy as np

EDT_INF = 2 ** 31 - 1            # UNETDC_EDT_INF
MAX_SIDE = 16384
MAX_RADIUS = 32767
DROPLET_QUANTITIES = ("cell", "n_in", "n_cells", "n_out", "area", "min_d2")                      # rows of out_droplet
CELL_QUANTITIES = ("area", "n_border", "fg_px", "n_droplets", "S_area", "S_area2", "max_area", "nucleus_px")   # rows of out_cell
_NONE = np.int64(1) << 40        # a column without a seed: above every finite squared distance


def check_radius(radius):
    """The territory radius in pixels: an integer 0..32767, 0 = unbounded (ValueError otherwise)."""
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"the cell radius is a whole number of pixels in 0..{MAX_RADIUS} (0: unbounded), not {radius!r}")
    return int(radius)


def check_flags(cell_dir, nuclei_dir, cell_radius, cell_labels):
    """The flags of the script, before any image is read -> "cells", "nuclei" or None (ValueError with the message of the
    argument error).  cell_radius: None when the flag was not given."""
    if cell_dir and nuclei_dir:
        raise ValueError("--cell_dir and --nuclei_dir are two sources of the same cells: give one")
    if cell_radius is not None and not nuclei_dir:
        raise ValueError("--cell_radius cuts the territories of nuclei: it needs --nuclei_dir")
    if cell_labels and not (cell_dir or nuclei_dir):
        raise ValueError("--cell_labels says how the masks of --cell_dir or --nuclei_dir are read: it needs one of them")
    if cell_radius is not None:
        check_radius(cell_radius)
    return "cells" if cell_dir else "nuclei" if nuclei_dir else None


def _column_pass(seed_label):
    """seed_label int64 [h, w], 0 = no seed -> (g2, gl): per pixel the minimum (dy^2, label) over the seeds of its column
    (_NONE, 0 without one).  One vector step per row, down with the last seed above, then up with the last seed below."""
    h, w = seed_label.shape
    d_dn, l_dn = np.empty((h, w), np.int64), np.empty((h, w), np.int64)
    d, l = np.full(w, -1, np.int64), np.zeros(w, np.int64)        # -1: no seed yet
    for y in range(h):
        s = seed_label[y]
        hit = s > 0
        d = np.where(hit, 0, np.where(d >= 0, d + 1, -1))
        l = np.where(hit, s, l)
        d_dn[y], l_dn[y] = d, l
    g, gl = np.empty((h, w), np.int64), np.empty((h, w), np.int64)
    d, l = np.full(w, -1, np.int64), np.zeros(w, np.int64)
    for y in range(h - 1, -1, -1):
        s = seed_label[y]
        hit = s > 0
        d = np.where(hit, 0, np.where(d >= 0, d + 1, -1))
        l = np.where(hit, s, l)
        a, la = d_dn[y], l_dn[y]
        up = (d >= 0) & ((a < 0) | (d < a) | ((d == a) & (l < la)))
        g[y], gl[y] = np.where(up, d, a), np.where(up, l, la)
    return np.where(g < 0, _NONE, g * g), gl


def nearest_label_numpy(label, max_label, radius=0):
    """label: integer [h, w] -> (out_label int32 [h, w], out_d2 int32 [h, w]) of unetdc_label_nearest.  The column pass keeps
    the minimum (dy^2, label) of every column; the row pass takes the minimum over x' of ((x - x')^2 + dy^2, label) as shifted
    planes, one pair of shifts per dx, for as long as dx^2 does not exceed the largest best distance of the image (a candidate
    at dx^2 == best can still win on its label)."""
    label = np.asarray(label)
    h, w = label.shape
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE) or max_label < 0:
        raise ValueError("nearest_label_numpy: sides 1..16384, a non-negative label limit")
    radius = check_radius(radius)
    lab = label.astype(np.int64)
    seed = np.where((lab >= 1) & (lab <= max_label), lab, 0)
    if not seed.any():
        return np.zeros((h, w), np.int32), np.full((h, w), EDT_INF, np.int32)
    g2, gl = _column_pass(seed)
    best, bl = g2.copy(), gl.copy()
    dx = 1
    while dx < w and dx * dx <= int(best.max()):
        dd = dx * dx
        for dst, src in ((slice(dx, w), slice(0, w - dx)), (slice(0, w - dx), slice(dx, w))):      # from the left, from the right
            c, cl = g2[:, src] + dd, gl[:, src]
            b, l = best[:, dst], bl[:, dst]
            take = (c < b) | ((c == b) & (cl < l))
            best[:, dst] = np.where(take, c, b)
            bl[:, dst] = np.where(take, cl, l)
        dx += 1
    assert int(best.max()) < EDT_INF                     # a seed exists: every pixel has found one within the row
    out_label = bl if radius == 0 else np.where(best > radius * radius, 0, bl)
    return out_label.astype(np.int32), best.astype(np.int32)


def cell_table_numpy(droplet_label, max_droplet, cell_label, max_cell, d2=None):
    """-> (out_droplet int32 [6, max_droplet], out_cell int64 [8, max_cell], needed) of unetdc_cell_table: rows in the order of
    DROPLET_QUANTITIES and CELL_QUANTITIES, needed = the number of (droplet, cell) pairs that share a pixel."""
    a = np.asarray(droplet_label).astype(np.int64)
    b = np.asarray(cell_label).astype(np.int64)
    if a.shape != b.shape or a.ndim != 2 or (d2 is not None and np.asarray(d2).shape != a.shape):
        raise ValueError("cell_table_numpy: the maps must be 2-D and of one size")
    h, w = a.shape
    a = np.where((a >= 1) & (a <= max_droplet), a, 0).ravel()
    b = np.where((b >= 1) & (b <= max_cell), b, 0).ravel()
    nd, nc = max_droplet + 1, max_cell + 1
    out_d, out_c = np.zeros((len(DROPLET_QUANTITIES), max_droplet), np.int64), np.zeros((len(CELL_QUANTITIES), max_cell), np.int64)
    out_d[5] = EDT_INF
    area = np.bincount(a, minlength=nd)[1:]
    out_d[4] = area
    out_d[3] = np.bincount(a[b == 0], minlength=nd)[1:]
    border = np.zeros((h, w), bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    out_c[0] = np.bincount(b, minlength=nc)[1:]
    out_c[1] = np.bincount(b[border.ravel()], minlength=nc)[1:]
    out_c[2] = np.bincount(b[a > 0], minlength=nc)[1:]
    if d2 is not None:
        d = np.asarray(d2).astype(np.int64).ravel()
        m = np.full(nd, EDT_INF, np.int64)
        np.minimum.at(m, a, d)
        out_d[5] = m[1:]
        out_c[7] = np.bincount(b[d == 0], minlength=nc)[1:]
    both = (a > 0) & (b > 0)
    keys, n = np.unique(a[both] * nc + b[both], return_counts=True)          # ascending (droplet, cell)
    ka, kb = keys // nc, keys % nc
    out_d[2] = np.bincount(ka, minlength=nd)[1:]
    # per droplet the triple with the largest n, the smallest cell at ties: the last of the order (droplet, n, -cell)
    order = np.lexsort((-kb, n, ka))
    last = np.ones(len(order), bool)
    last[:-1] = ka[order][1:] != ka[order][:-1]
    win = order[last]
    out_d[0, ka[win] - 1], out_d[1, ka[win] - 1] = kb[win], n[win]
    k = np.flatnonzero(out_d[0] > 0)
    cell, ar = out_d[0, k], area[k]
    out_c[3] = np.bincount(cell, minlength=nc)[1:]
    np.add.at(out_c[4], cell - 1, ar)
    np.add.at(out_c[5], cell - 1, ar * ar)
    np.maximum.at(out_c[6], cell - 1, ar)
    return out_d.astype(np.int32), out_c, int(len(keys))


def cells_record(droplet_label, n_droplets, cell_label, max_cell, d2=None):
    """The record the droplet stage keeps per image (Droplets.cells), from host arrays: the DROPLET_QUANTITIES as int64 [n]
    by name, "cells": the CELL_QUANTITIES as int64 [max_cell] by name, "nuclei": whether d2 was given."""
    out_d, out_c, _ = cell_table_numpy(droplet_label, n_droplets, cell_label, max_cell, d2)
    return make_record(out_d.astype(np.int64), out_c, d2 is not None)


def make_record(out_droplet, out_cell, nuclei):
    return {**dict(zip(DROPLET_QUANTITIES, out_droplet)), "cells": dict(zip(CELL_QUANTITIES, out_cell)), "nuclei": bool(nuclei)}


# ---- columns ------------------------------------------------------------------------------------------------------------------

def original_ids(cell, ids):
    """Cell numbers 0..K (any shape) -> the numbers of the file they were renumbered from (ids [K], ascending); ids None: as they are."""
    cell = np.asarray(cell)
    return cell if ids is None else np.concatenate([[0], np.asarray(ids, np.int64)])[cell]


def cell_columns(rec, px_per_um=None, ids=None):
    """The per-droplet columns behind the table's own, in their order in the CSV: cell, cell_overlap_frac (n_in / area),
    n_cells, outside_cells (cell == 0); with nuclei also nucleus_gap_px = sqrt(min_d2), 0 when the droplet touches the nucleus
    (NaN when there is no nucleus in the image), and its micron twin."""
    cell, n_in, area = (np.asarray(rec[q], np.int64) for q in ("cell", "n_in", "area"))
    cols = {"cell": original_ids(cell, ids), "cell_overlap_frac": n_in / np.maximum(area, 1), "n_cells": np.asarray(rec["n_cells"], np.int64),
            "outside_cells": cell == 0}
    if rec["nuclei"]:
        m = np.asarray(rec["min_d2"], np.int64)
        cols["nucleus_gap_px"] = np.array([math.sqrt(v) if v != EDT_INF else math.nan for v in m.tolist()], dtype=np.float64)
        if px_per_um is not None:
            cols["nucleus_gap_um"] = cols["nucleus_gap_px"] / px_per_um
    return cols


def cells_table(filename, rec, px_per_um=None, ids=None):
    """One image's rows of cells.csv as a dict of columns: one row per cell label that owns a pixel.  Mean and standard
    deviation (population) of the assigned droplets' areas come from the device's integer sums, the median from the droplet
    table on the host."""
    c = {q: np.asarray(v, np.int64) for q, v in rec["cells"].items()}
    rows = np.flatnonzero(c["area"] > 0)
    area, n, S, S2 = (c[q][rows].tolist() for q in ("area", "n_droplets", "S_area", "S_area2"))
    d_cell, d_area = np.asarray(rec["cell"], np.int64), np.asarray(rec["area"], np.int64)
    median = [float(np.median(d_area[d_cell == k + 1])) if c["n_droplets"][k] else math.nan for k in rows]
    mean = [s / m if m else math.nan for s, m in zip(S, n)]
    std = [math.sqrt(max(m * s2 - s * s, 0)) / m if m else math.nan for s, s2, m in zip(S, S2, n)]
    cols = {"filename": [filename] * len(rows), "cell": original_ids(rows + 1, ids), "area_px": c["area"][rows]}
    if px_per_um is not None:
        cols["area_um2"] = c["area"][rows] / (px_per_um * px_per_um)
    cols.update({"touches_border": c["n_border"][rows] > 0, "n_droplets": c["n_droplets"][rows], "droplet_area_px": c["fg_px"][rows],
                 "droplet_area_frac": np.array([f / a for f, a in zip(c["fg_px"][rows].tolist(), area)], dtype=np.float64),
                 "droplet_mean_area_px": np.array(mean, dtype=np.float64), "droplet_std_area_px": np.array(std, dtype=np.float64),
                 "droplet_median_area_px": np.array(median, dtype=np.float64), "droplet_max_area_px": c["max_area"][rows]})
    if rec["nuclei"]:
        cols["nucleus_area_px"] = c["nucleus_px"][rows]
    return cols


SUMMARY_NAMES = ("n_cells", "n_cells_whole", "droplets_per_cell_mean", "droplets_per_cell_median", "frac_cells_without_droplets",
                 "n_droplets_outside_cells")


def per_image_summary(rec):
    """The numbers a row of cells_per_image.csv and of summary_per_image.csv gains (SUMMARY_NAMES).  A cell is a label that owns
    a pixel; a whole cell has no pixel on the image border.  The droplets per cell and the share of cells without droplets are
    taken over the whole cells (a cell cut by the border has lost droplets with the part outside); NaN without one."""
    c = rec["cells"]
    area, nb, nd = (np.asarray(c[q], np.int64) for q in ("area", "n_border", "n_droplets"))
    cells = area > 0
    whole = cells & (nb == 0)
    per = nd[whole]
    return {"n_cells": int(cells.sum()), "n_cells_whole": int(whole.sum()),
            "droplets_per_cell_mean": float(per.mean()) if len(per) else math.nan,
            "droplets_per_cell_median": float(np.median(per)) if len(per) else math.nan,
            "frac_cells_without_droplets": float((per == 0).mean()) if len(per) else math.nan,
            "n_droplets_outside_cells": int((np.asarray(rec["cell"]) == 0).sum())}
