"""Boundary accuracy of a predicted label map against an annotated one: surface distances.

``boundary_record_numpy`` is the host path of what ``unetdc_boundary_distances`` computes on the device: for every boundary
pixel of one map the exact squared distance to the nearest boundary pixel of the other, as a histogram up to R^2 (+ "far"), the
largest squared distance per direction and count / max / sum per object.  The record is all integers.  ``boundary_columns`` is
the ONE place where a record becomes Hausdorff distance, HD95, ASSD, surface Dice and boundary precision / recall / F, for
the device path, the CPU path and the tests alike; ``object_columns`` does the same for the per-object rows; ``summary_row``
and ``pooled_row`` build the rows of ``boundary_per_image.csv``.

A per-object distance runs to the nearest boundary pixel of ANY object of the other map, not to that of a matched partner.
"""
import math

import numpy as np

EDT_INF = 2147483647              # UNETDC_EDT_INF: no boundary pixel on the other map
MAX_RADIUS = 64
DEFAULT_RADIUS = 64
DEFAULT_TOLS = (1, 2, 3)
OBJECT_COLUMNS = ("bd_px", "bd_rms", "bd_max")


def check_radius(R):
    if not (isinstance(R, (int, np.integer)) and 1 <= int(R) <= MAX_RADIUS):
        raise ValueError(f"the boundary radius must be an integer in 1..{MAX_RADIUS}, not {R!r}")
    return int(R)


def check_tols(tols, R):
    tols = tuple(int(t) for t in tols)
    if not tols or any(t < 0 or t > R for t in tols) or len(set(tols)) != len(tols):
        raise ValueError(f"boundary tolerances must be distinct integers in 0..{R}, not {tols!r}")
    return tols


def range_rule(L, k):
    """int label map -> int64 map in which every value below 1 or above k is 0."""
    a = np.asarray(L).astype(np.int64)
    return np.where((a >= 1) & (a <= int(k)), a, 0)


def boundary_mask(L, k):
    """bool [h, w]: the pixels that carry a label in 1..k and have a 4-neighbour outside the image or of another value (after
    the range rule).  The cut between two touching objects is boundary, and so is the frame of the image."""
    a = range_rule(L, k)
    p = np.pad(a, 1, constant_values=-1)
    other = (p[:-2, 1:-1] != a) | (p[2:, 1:-1] != a) | (p[1:-1, :-2] != a) | (p[1:-1, 2:] != a)
    return (a >= 1) & other


def _d2_to(mask_to):
    """int64 [h, w]: the exact squared distance of every pixel to the nearest True pixel of mask_to, EDT_INF without one."""
    if not mask_to.any():
        return np.full(mask_to.shape, EDT_INF, np.int64)
    from scipy import ndimage
    d = ndimage.distance_transform_edt(~mask_to)
    return np.rint(d * d).astype(np.int64)               # d^2 < 2^29 is an integer: the float64 square is off by far less than 1/2


def _table(lab, d2, k):
    out = np.zeros((3, k), np.int64)
    out[1] = -1
    if len(lab):
        out[0] = np.bincount(lab, minlength=k + 1)[1:k + 1]
        np.maximum.at(out[1], lab - 1, d2)
        np.add.at(out[2], lab - 1, d2)
    return out


def boundary_record_numpy(A, ka, B, kb, R, objects=True):
    """A (the prediction), B (the annotation): int label maps of one shape, objects 1..ka and 1..kb.  -> dict:
      hist  int64 [2, R^2 + 2]: hist[0][min(d2, R^2 + 1)] counts the boundary pixels of A by their squared distance to the
            boundary of B, hist[1] the mirror; bin R^2 + 1 is "far";
      dmax  int64 [2]: the largest squared distance per direction, unclamped, -1 without a boundary pixel;
      a, b  int64 [3, ka], [3, kb] (None without objects): per object count, max d2 (-1 without a pixel), sum of d2."""
    R = check_radius(R)
    A, B = np.asarray(A), np.asarray(B)
    if A.shape != B.shape or A.ndim != 2:
        raise ValueError("the two label maps differ in size")
    ka, kb = int(ka), int(kb)
    la, lb = range_rule(A, ka), range_rule(B, kb)
    ba, bb = boundary_mask(A, ka), boundary_mask(B, kb)
    far = R * R + 1
    hist, dmax, tables = np.zeros((2, far + 1), np.int64), np.full(2, -1, np.int64), []
    for d, (mine, other, lab, k) in enumerate(((ba, bb, la, ka), (bb, ba, lb, kb))):
        d2 = _d2_to(other)[mine]
        hist[d] = np.bincount(np.minimum(d2, far), minlength=far + 1)
        if len(d2):
            dmax[d] = d2.max()
        tables.append(_table(lab[mine], d2, k) if objects else None)
    return {"hist": hist, "dmax": dmax, "a": tables[0], "b": tables[1]}


def _ratio(num, den, nothing):
    """A ratio with a zero denominator is 0.0 -- but where neither map holds a boundary pixel, every ratio is 1.0."""
    return 1.0 if nothing else (num / den if den else 0.0)


def _percentile_bin(row, n):
    """Nearest rank: the smallest bin whose cumulative count reaches ceil(95 n / 100), in integers."""
    return int(np.searchsorted(np.cumsum(row), (95 * n + 99) // 100, side="left"))


def boundary_columns(hist, dmax, R, tols=DEFAULT_TOLS):
    """The record's integers -> the float64 columns (a dict in column order).  hd = sqrt(max dmax), inf when a side has boundary
    pixels and the other none, 0.0 when both are empty.  hd95: per direction the nearest-rank 95th percentile of the clamped
    histogram as sqrt(min(bin, R^2)), the larger of the two; a value equal to R with far pixels reads "at least R".  assd: the
    mean of sqrt(min(bin, R^2)) over all boundary pixels of both maps (far pixels count with R; 0.0 when both are empty).  Per
    tolerance t, with c = the pixels within t (d2 <= t^2): bprec = c0 / n0, brec = c1 / n1, bf = their harmonic mean in
    integers, nsd = (c0 + c1) / (n0 + n1)."""
    R = check_radius(R)
    tols = check_tols(tols, R)
    hist = np.asarray(hist, dtype=np.int64)
    if hist.shape != (2, R * R + 2):
        raise ValueError(f"hist must be [2, {R * R + 2}]")
    n = [int(hist[0].sum()), int(hist[1].sum())]
    nothing = n[0] == 0 and n[1] == 0
    top = max(int(dmax[0]), int(dmax[1]))
    out = {"bd_px_pred": n[0], "bd_px_gt": n[1], "n_far_pred": int(hist[0, -1]), "n_far_gt": int(hist[1, -1])}
    out["hd"] = 0.0 if nothing else (math.inf if top >= EDT_INF else math.sqrt(top))
    out["hd95"] = max(math.sqrt(min(_percentile_bin(hist[d], n[d]), R * R)) if n[d] else 0.0 for d in (0, 1))
    terms = [int(hist[d, l]) * math.sqrt(min(l, R * R)) for d in (0, 1) for l in np.flatnonzero(hist[d]).tolist()]
    out["assd"] = math.fsum(terms) / (n[0] + n[1]) if not nothing else 0.0
    for t in tols:
        c0, c1 = int(hist[0, :t * t + 1].sum()), int(hist[1, :t * t + 1].sum())
        out[f"bprec_{t}"] = _ratio(c0, n[0], nothing)
        out[f"brec_{t}"] = _ratio(c1, n[1], nothing)
        out[f"bf_{t}"] = _ratio(2 * c0 * c1, c0 * n[1] + c1 * n[0], nothing)
        out[f"nsd_{t}"] = _ratio(c0 + c1, n[0] + n[1], nothing)
    return out


def column_names(tols=DEFAULT_TOLS):
    return ["filename", "bd_px_pred", "bd_px_gt", "n_far_pred", "n_far_gt", "hd", "hd95", "assd"] + \
        [f"{q}_{t}" for t in tols for q in ("bprec", "brec", "bf", "nsd")]


def object_columns(table):
    """int64 [3, k] (count, max d2, sum d2) -> {"bd_px": int64 [k], "bd_rms": sqrt(sum / count), "bd_max": sqrt(max)}, both
    float64: inf where the other map has no boundary pixel, NaN (an empty CSV cell) for an object without a boundary pixel."""
    t = np.asarray(table, dtype=np.int64).reshape(3, -1)
    some = t[0] > 0
    inf = some & (t[1] >= EDT_INF)
    fin = some & ~inf                                    # there the sum is below 2^53: the conversions to float64 are exact
    rms, mx = np.full(t.shape[1], np.nan), np.full(t.shape[1], np.nan)
    rms[fin] = np.sqrt(t[2][fin].astype(np.float64) / t[0][fin].astype(np.float64))
    mx[fin] = np.sqrt(t[1][fin].astype(np.float64))
    rms[inf] = mx[inf] = math.inf
    return {"bd_px": t[0].copy(), "bd_rms": rms, "bd_max": mx}


def summary_row(filename, hist, dmax, R, tols=DEFAULT_TOLS):
    """One row of boundary_per_image.csv."""
    return {"filename": filename, **boundary_columns(hist, dmax, R, tols)}


def pooled_row(records, R, tols=DEFAULT_TOLS, filename="ALL"):
    """The row of the summed histograms and the largest dmax of the (hist, dmax) pairs: its ratios come from those integers,
    not from the images' ratios."""
    hist, dmax = np.zeros((2, R * R + 2), np.int64), np.full(2, -1, np.int64)
    for h, d in records:
        hist += np.asarray(h, dtype=np.int64)
        dmax = np.maximum(dmax, np.asarray(d, dtype=np.int64))
    return summary_row(filename, hist, dmax, R, tols)
