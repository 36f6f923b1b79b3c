"""Per-droplet shape and intensity columns.

``label_props_numpy`` is the host path of what ``unetdc_ccl_labels`` / ``unetdc_split_stats`` + ``unetdc_label_props``
compute on the device: exact integers per label of an int32 label map.  ``shape_columns`` is the ONE place where those
integers become the float64 columns of the droplet table, for the device path, the CPU path and the tests alike.
"""
import math

import numpy as np

# the rows of unetdc_label_props, in its order (include/unetdc_hip.h)
QUANTITIES = ("Syy", "Sxx", "Sxy", "min_y", "min_x", "max_y", "max_x", "P1", "P2", "P3", "Sg", "Sgg", "min_g", "max_g")
GRAY_QUANTITIES = QUANTITIES[10:]
MIN_INIT, MAX_INIT = 2 ** 63 - 1, -1         # what a label without pixels keeps in a minimum / maximum row

PERIMETER_CLASSES = ((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))
PERIMETER_WEIGHTS = (1.0, math.sqrt(2.0), (1.0 + math.sqrt(2.0)) / 2.0)


def border_codes(labels):
    """int64 [h, w]: 0 where a pixel is background or no border pixel of its label, else 1 + 2 * (border 4-neighbours of
    the same label) + 10 * (border diagonal neighbours of the same label); the outside of the image has no label."""
    lab = np.asarray(labels)
    h, w = lab.shape
    p = np.full((h + 4, w + 4), -1, np.int64)
    p[2:-2, 2:-2] = lab
    c = p[1:-1, 1:-1]                                      # one pixel of margin around the image
    inner = (p[:-2, 1:-1] == c) & (p[2:, 1:-1] == c) & (p[1:-1, :-2] == c) & (p[1:-1, 2:] == c)
    border = (c > 0) & ~inner
    code = np.zeros((h, w), np.int64)
    centre = c[1:-1, 1:-1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            sl = (slice(1 + dy, 1 + dy + h), slice(1 + dx, 1 + dx + w))
            code += (border[sl] & (c[sl] == centre)) * (10 if dy and dx else 2)
    return np.where(border[1:-1, 1:-1], code + 1, 0)


def _per_label(order, starts, present, k, values, ufunc, init):
    out = np.full(k, init, np.int64)
    if len(starts):
        out[present - 1] = ufunc.reduceat(values[order], starts)
    return out


def label_props_numpy(labels, gray=None):
    """labels: int [h, w], 0 = background, droplets 1..K (K = labels.max()); gray: uint8 [h, w] or None.
    -> dict of int64 arrays [K]: area, Sy, Sx and QUANTITIES (the four grey ones only with a grey plane).  Exact: int64
    sums over the pixels of each label, sorted by label."""
    lab = np.asarray(labels)
    h, w = lab.shape
    k = int(lab.max(initial=0))
    flat = lab.ravel()
    idx = np.flatnonzero(flat > 0)
    order = np.argsort(flat[idx], kind="stable")
    idx = idx[order]
    present, starts = np.unique(flat[idx], return_index=True)
    present = present.astype(np.int64)
    ident = np.arange(len(idx))
    y, x = (idx // w).astype(np.int64), (idx % w).astype(np.int64)

    def red(values, ufunc=np.add, init=0):
        return _per_label(ident, starts, present, k, values, ufunc, init)

    out = {"area": red(np.ones(len(idx), np.int64)), "Sy": red(y), "Sx": red(x), "Syy": red(y * y), "Sxx": red(x * x),
           "Sxy": red(x * y), "min_y": red(y, np.minimum, MIN_INIT), "min_x": red(x, np.minimum, MIN_INIT),
           "max_y": red(y, np.maximum, MAX_INIT), "max_x": red(x, np.maximum, MAX_INIT)}
    code = border_codes(lab).ravel()[idx]
    for name, codes in zip(("P1", "P2", "P3"), PERIMETER_CLASSES):
        out[name] = red(np.isin(code, codes).astype(np.int64))
    if gray is not None:
        g = np.asarray(gray).ravel()[idx].astype(np.int64)
        out.update(Sg=red(g), Sgg=red(g * g), min_g=red(g, np.minimum, MIN_INIT), max_g=red(g, np.maximum, MAX_INIT))
    return out


def _ratio(num, den):
    """Exact integer numerators and denominators (Python integers) -> correctly rounded float64 quotients."""
    return np.array([n / d for n, d in zip(num, den)], dtype=np.float64)


def shape_columns(props, hw, px_per_um=None):
    """props: the integers of label_props_numpy (or of the device path) for droplets that each have at least one pixel;
    hw: (h, w) of the image.  -> dict of the table's extra columns, in their order in the CSV."""
    h, w = int(hw[0]), int(hw[1])
    A, Sy, Sx, Syy, Sxx, Sxy = ([int(v) for v in props[q]] for q in ("area", "Sy", "Sx", "Syy", "Sxx", "Sxy"))
    n = len(A)
    den = [a * a for a in A]
    nr = [a * s2 - s * s for a, s2, s in zip(A, Syy, Sy)]                  # exact: they pass 2^63 on large images
    nc = [a * s2 - s * s for a, s2, s in zip(A, Sxx, Sx)]
    nv = [a * sxy - sy * sx for a, sxy, sy, sx in zip(A, Sxy, Sy, Sx)]
    vr, vc, cv = _ratio(nr, den), _ratio(nc, den), _ratio(nv, den)
    mid, half = (vr + vc) / 2.0, np.hypot((vc - vr) / 2.0, cv)
    l1, l2 = np.maximum(mid + half, 0.0), np.maximum(mid - half, 0.0)
    round_ = np.array([v == 0 and a == b for v, a, b in zip(nv, nr, nc)], dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        ecc = np.where(l1 > 0, np.sqrt(np.maximum(1.0 - l2 / np.where(l1 > 0, l1, 1.0), 0.0)), 0.0)
    # a zero covariance is +0.0 here (0 / A^2), so a droplet wider than tall reads atan2(+0, negative) / 2 = +pi / 2
    orientation = np.where(round_, -math.pi / 4.0, 0.5 * np.arctan2(2.0 * cv, vr - vc))
    p1, p2, p3 = (np.asarray(props[q], dtype=np.float64) for q in ("P1", "P2", "P3"))
    perimeter = PERIMETER_WEIGHTS[0] * p1 + PERIMETER_WEIGHTS[1] * p2 + PERIMETER_WEIGHTS[2] * p3
    area = np.asarray(A, dtype=np.float64)
    circ = np.where(perimeter > 0, 4.0 * math.pi * area / np.where(perimeter > 0, perimeter, 1.0) ** 2, 0.0)
    miny, minx, maxy, maxx = (np.asarray(props[q], dtype=np.int64) for q in ("min_y", "min_x", "max_y", "max_x"))
    cols = {"perimeter": perimeter, "circularity": circ, "axis_major_length": 4.0 * np.sqrt(l1),
            "axis_minor_length": 4.0 * np.sqrt(l2), "eccentricity": ecc, "orientation": orientation,
            "bbox-0": miny, "bbox-1": minx, "bbox-2": maxy + 1, "bbox-3": maxx + 1,
            "touches_border": (miny == 0) | (minx == 0) | (maxy == h - 1) | (maxx == w - 1)}
    if "Sg" in props:
        Sg, Sgg = ([int(v) for v in props[q]] for q in ("Sg", "Sgg"))
        cols["intensity_mean"] = _ratio(Sg, A)
        cols["intensity_min"] = np.asarray(props["min_g"], dtype=np.int64)
        cols["intensity_max"] = np.asarray(props["max_g"], dtype=np.int64)
        cols["intensity_std"] = np.array([math.sqrt(max(a * s2 - s * s, 0)) / a for a, s2, s in zip(A, Sgg, Sg)], dtype=np.float64)
    if px_per_um is not None:
        cols["perimeter_micron"] = perimeter / px_per_um
        cols["axis_major_micron"] = cols["axis_major_length"] / px_per_um
        cols["axis_minor_micron"] = cols["axis_minor_length"] / px_per_um
    assert all(len(v) == n for v in cols.values())
    return cols
