"""Convex hull, solidity and Feret diameters per droplet.

The point set of a label is the union of the closed unit squares [x, x + 1] x [y, y + 1] of its pixels (y, x); its convex hull
has lattice vertices and is listed without collinear points.  ``label_hull_numpy`` is the host path of what
``unetdc_label_hull`` computes on the device: five exact integers per label of an int32 label map.  ``hull_columns`` is the
ONE place where those integers become the float64 columns of the droplet table, for the device path, the CPU path and the
tests alike.
"""
import math

import numpy as np

# the rows of unetdc_label_hull, in its order (include/unetdc_hip.h)
QUANTITIES = ("H2", "F2", "Wc", "Wl", "nv")
COLUMN_NAMES = ("area_convex", "solidity", "feret_diameter_max", "feret_diameter_min", "feret_ratio", "hull_vertices",
                "low_solidity")
MICRON_COLUMN_NAMES = ("feret_max_micron", "feret_min_micron", "area_convex_sqmicron")
SUMMARY_NAMES = ("solidity_median", "feret_max_median", "n_low_solidity")
DEFAULT_SOLIDITY = 0.9


def check_solidity(s):
    """The threshold of the low_solidity flag: 0 < S <= 1."""
    s = float(s)
    if not 0.0 < s <= 1.0:
        raise ValueError(f"the solidity threshold must lie in (0, 1], got {s}")
    return s


def _chain(ts, xs, sign):
    """Monotone chain over the points (xs[i], ts[i]), ts ascending: sign = +1 the left chain of the hull (the lower hull of
    (t, x)), -1 the right one.  Collinear points are dropped.  -> list of (x, t)."""
    st = []
    for t, x in zip(ts, xs):
        while len(st) >= 2:
            (ox, ot), (ax, at) = st[-2], st[-1]
            if sign * ((at - ot) * (x - ox) - (ax - ox) * (t - ot)) > 0:
                break
            st.pop()
        st.append((x, t))
    return st


def hull_of_rows(y0, xl, xr):
    """xl, xr: the leftmost and rightmost pixel column of the rows y0, y0 + 1, ... of one label (-1 in both for a row without
    a pixel; the first and the last row have one) -> the hull's vertices [(x, y), ...] as Python integers: the left chain
    top to bottom, then the right chain bottom to top."""
    xl, xr = np.asarray(xl, np.int64), np.asarray(xr, np.int64)
    big = np.iinfo(np.int64).max
    lo = np.where(xr >= 0, xl, big)
    left = np.minimum(np.concatenate((lo, [big])), np.concatenate(([big], lo)))          # per corner level
    right = np.maximum(np.concatenate((xr, [-1])), np.concatenate(([-1], xr))) + 1
    t = np.flatnonzero(right > 0)
    ts = (t + y0).tolist()
    return _chain(ts, left[t].tolist(), 1) + _chain(ts, right[t].tolist(), -1)[::-1]


def hull_integers(v):
    """v: the hull's vertices in order, Python integers -> (H2, F2, Wc, Wl, nv).  Brute force over all pairs, vectorised."""
    n = len(v)
    x, y = np.array([p[0] for p in v], np.int64), np.array([p[1] for p in v], np.int64)
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    h2 = abs(int(np.sum(x * yn - xn * y)))
    f2 = int(((x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2).max())
    ex, ey = xn - x, yn - y
    wc = np.abs(ex[:, None] * (y[None, :] - y[:, None]) - ey[:, None] * (x[None, :] - x[:, None])).max(axis=1)
    wl = ex * ex + ey * ey
    best = None
    for c, l in zip(wc.tolist(), wl.tolist()):                  # exact: Python integers
        if best is None or (c * c * best[1], l) < (best[0] * best[0] * l, best[1]):
            best = (c, l)
    return h2, f2, best[0], best[1], n


def label_hull_numpy(labels, max_out=None):
    """labels: int [h, w], 0 = background, droplets 1..max_out (default labels.max()); labels outside that are skipped.
    -> dict of int64 arrays [max_out] under QUANTITIES; a label without pixels keeps 0 everywhere.  The per-(label, row)
    extents come from one sort of the droplet pixels; the chain and the calipers run per label."""
    lab = np.asarray(labels)
    h, w = lab.shape
    k = int(lab.max(initial=0)) if max_out is None else int(max_out)
    out = {q: np.zeros(k, np.int64) for q in QUANTITIES}
    flat = lab.ravel()
    idx = np.flatnonzero((flat > 0) & (flat <= k))
    if not len(idx):
        return out
    key = flat[idx].astype(np.int64) * h + idx // w                 # (label, row), ascending within a label
    order = np.argsort(key, kind="stable")
    key, x = key[order], (idx % w)[order]
    rows, starts = np.unique(key, return_index=True)
    xl, xr = np.minimum.reduceat(x, starts), np.maximum.reduceat(x, starts)
    lab_of, y_of = rows // h, rows % h
    present, first = np.unique(lab_of, return_index=True)
    last = np.append(first[1:], len(rows))
    for lbl, a, b in zip(present.tolist(), first.tolist(), last.tolist()):
        y0, height = int(y_of[a]), int(y_of[b - 1] - y_of[a] + 1)
        l, r = np.full(height, -1, np.int64), np.full(height, -1, np.int64)
        l[y_of[a:b] - y0], r[y_of[a:b] - y0] = xl[a:b], xr[a:b]
        for q, val in zip(QUANTITIES, hull_integers(hull_of_rows(y0, l, r))):
            out[q][lbl - 1] = val
    return out


def hull_columns(hull, area, solidity_below=DEFAULT_SOLIDITY, px_per_um=None):
    """hull: the integers of label_hull_numpy (or of the device path) for droplets that each have at least one pixel; area:
    their pixel counts.  -> dict of the table's extra columns, in their order in the CSV.  Ratios of integers are one
    correctly rounded division of Python integers."""
    A = [int(v) for v in area]
    H2, F2, Wc, Wl, nv = ([int(v) for v in hull[q]] for q in QUANTITIES)
    solidity = np.array([2 * a / h2 for a, h2 in zip(A, H2)], dtype=np.float64)
    fmax = np.array([math.sqrt(f) for f in F2], dtype=np.float64)
    fmin = np.array([math.sqrt(c * c / l) for c, l in zip(Wc, Wl)], dtype=np.float64)
    cols = {"area_convex": np.array([h2 / 2 for h2 in H2], dtype=np.float64), "solidity": solidity,
            "feret_diameter_max": fmax, "feret_diameter_min": fmin, "feret_ratio": fmin / fmax if len(A) else fmin,
            "hull_vertices": np.asarray(nv, dtype=np.int64), "low_solidity": solidity < check_solidity(solidity_below)}
    if px_per_um is not None:
        cols["feret_max_micron"] = fmax / px_per_um
        cols["feret_min_micron"] = fmin / px_per_um
        cols["area_convex_sqmicron"] = cols["area_convex"] / (px_per_um * px_per_um)
    assert tuple(cols)[:len(COLUMN_NAMES)] == COLUMN_NAMES and all(len(v) == len(A) for v in cols.values())
    return cols


def hull_summary(cols):
    """The three per-image summary values of SUMMARY_NAMES from hull_columns' result (NaN medians without a droplet)."""
    n = len(cols["solidity"])
    return {"solidity_median": float(np.median(cols["solidity"])) if n else float("nan"),
            "feret_max_median": float(np.median(cols["feret_diameter_max"])) if n else float("nan"),
            "n_low_solidity": int(np.count_nonzero(cols["low_solidity"]))}
