"""Splitting touching droplets on the host: the definition of DESIGN.md ("Splitting touching droplets") on numpy / scipy.

    1. D2[p]   exact squared Euclidean distance to the nearest background pixel inside the image (int32, 0 on
               background; EDT_INF everywhere when the mask has no background pixel)
    2. basins  every foreground pixel points to the largest key (D2, -index) among itself and its foreground
               4-neighbours; pixels whose pointer chains end in the same pixel form a basin, peak = D2 there
    3. merging 4-adjacent foreground pixels p, q of different basins A, B are united iff, with S = min(D2[p], D2[q]),
               P = min(peak(A), peak(B)), H2 the split depth in half pixels:  t = 4P - 4S - H2^2 <= 0  or
               t^2 <= 16 H2^2 S   (sqrt(P) - sqrt(S) <= H2 / 2 in integers).  The test looks at one pixel pair only, so
               the classes do not depend on any order
    4. droplets the classes with at least max(min_area, 1) pixels, numbered in raster order of their first pixel

This module is the CPU path of ``quantify_droplets_batch.py --split_touching`` and the yardstick of the HIP kernels
(csrc/split.hip, tests/test_gpu_split.py); tests/split_ref.py restates the same four steps in plain loops.
"""
from __future__ import annotations

import numpy as np

EDT_INF = 2 ** 31 - 1       # UNETDC_EDT_INF
MAX_SIDE = 16384            # as the kernels: D2 < 2^29, the merge test stays inside 64 bits


def half_pixels(split_depth):
    """Split depth in pixels (a non-negative multiple of 0.5) -> H2, the depth in half pixels; ValueError otherwise."""
    d = float(split_depth)
    if not (d >= 0.0) or d != d or d == float("inf") or (2.0 * d) != int(2.0 * d):
        raise ValueError("the split depth must be a non-negative multiple of 0.5 pixels")
    return int(2.0 * d)


def edt_sq(mask):
    """Step 1.  scipy's feature transform gives the nearest background pixel of every pixel (integer arithmetic inside, so
    the pixel is a true nearest one); the squared distance to it is formed here in integers."""
    from scipy import ndimage
    fg = np.asarray(mask) != 0
    h, w = fg.shape
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError("image sides above 16384 are not supported")
    if fg.all():
        return np.full((h, w), EDT_INF, np.int32)
    idx = ndimage.distance_transform_edt(fg, return_distances=False, return_indices=True)
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (idx[0].astype(np.int64) - yy) ** 2 + (idx[1].astype(np.int64) - xx) ** 2
    return d2.astype(np.int32)


def basins(fg, d2):
    """Step 2 -> int64 [h, w]: the linear index of every foreground pixel's basin root (its own index on background)."""
    h, w = fg.shape
    n = h * w
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    best_d = np.where(fg, d2.astype(np.int64), -1)
    best_i = idx.copy()
    cand_d = np.where(fg, d2.astype(np.int64), -1)
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        nd = np.full((h, w), -1, np.int64)                 # neighbour's D2, -1 where it is background or outside
        ni = np.zeros((h, w), np.int64)
        ys, yd = (slice(0, h - 1), slice(1, h)) if dy < 0 else (slice(1, h), slice(0, h - 1)) if dy > 0 else (slice(None),) * 2
        xs, xd = (slice(0, w - 1), slice(1, w)) if dx < 0 else (slice(1, w), slice(0, w - 1)) if dx > 0 else (slice(None),) * 2
        nd[yd, xd] = cand_d[ys, xs]
        ni[yd, xd] = idx[ys, xs]
        better = fg & ((nd > best_d) | ((nd == best_d) & (ni < best_i)))
        best_d = np.where(better, nd, best_d)
        best_i = np.where(better, ni, best_i)
    ptr = best_i.ravel()
    while True:                                            # pointer doubling: keys grow along a chain, so it ends
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            return ptr.reshape(h, w)
        ptr = nxt


def split_labels(mask, split_depth_half_px, min_area=1):
    """Steps 1-4 -> (labels int32 [h, w] with 0 = background or dropped, area int64 [n], sum_row int64 [n],
    sum_col int64 [n], first_pixel int64 [n]) -- what unetdc_split_stats computes."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    fg = np.asarray(mask) != 0
    h, w = fg.shape
    n = h * w
    h2 = int(split_depth_half_px)
    if h2 < 0:
        raise ValueError("negative split depth")
    h2 = min(h2, 2 * (h + w))                              # from there on every pair passes anyway
    empty = (np.zeros((h, w), np.int32),) + tuple(np.zeros(0, np.int64) for _ in range(4))
    if not fg.any():
        return empty
    d2 = edt_sq(fg).astype(np.int64)
    root = basins(fg, d2)
    peak = d2.ravel()[root]
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    ea, eb = [], []
    for a, b in (((slice(None), slice(0, w - 1)), (slice(None), slice(1, w))),
                 ((slice(0, h - 1), slice(None)), (slice(1, h), slice(None)))):
        both = fg[a] & fg[b]
        p, q = idx[a][both], idx[b][both]
        same = root[a][both] == root[b][both]
        S = np.minimum(d2[a][both], d2[b][both])
        P = np.minimum(peak[a][both], peak[b][both])
        t = 4 * P - 4 * S - h2 * h2
        tp = np.where(t > 0, t, 0).astype(np.uint64)       # t > 0 means H2^2 < 4P < 2^31: both sides fit 64 bits
        ok = same | (t <= 0) | ((t > 0) & (tp * tp <= np.uint64(16 * h2 * h2) * S.astype(np.uint64)))
        ea.append(p[ok])
        eb.append(q[ok])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    fidx = np.flatnonzero(fg.ravel())
    comp = np.full(n, -1, np.int64)
    comp[fidx] = np.arange(len(fidx))
    g = coo_matrix((np.ones(len(ea), np.int8), (comp[ea], comp[eb])), shape=(len(fidx), len(fidx)))
    ncls, cls = connected_components(g, directed=False)
    area = np.bincount(cls, minlength=ncls)
    first = np.full(ncls, n, np.int64)
    np.minimum.at(first, cls, fidx)
    keep = np.flatnonzero(area >= max(int(min_area), 1))
    keep = keep[np.argsort(first[keep], kind="stable")]
    if len(keep) == 0:
        return empty
    number = np.zeros(ncls, np.int32)
    number[keep] = np.arange(1, len(keep) + 1, dtype=np.int32)
    labels = np.zeros(n, np.int32)
    labels[fidx] = number[cls]
    sy = np.zeros(ncls, np.int64)
    sx = np.zeros(ncls, np.int64)
    np.add.at(sy, cls, fidx // w)
    np.add.at(sx, cls, fidx % w)
    return labels.reshape(h, w), area[keep].astype(np.int64), sy[keep], sx[keep], first[keep]


def label_boundaries(labels):
    """Pixels with a 4-neighbour of another nonzero label: the cuts, for the overlay."""
    lab = np.asarray(labels)
    out = np.zeros(lab.shape, bool)
    d = (lab[:, 1:] != lab[:, :-1]) & (lab[:, 1:] > 0) & (lab[:, :-1] > 0)
    out[:, 1:] |= d
    out[:, :-1] |= d
    d = (lab[1:] != lab[:-1]) & (lab[1:] > 0) & (lab[:-1] > 0)
    out[1:] |= d
    out[:-1] |= d
    return out


def labels_u16(labels):
    """The 16-bit image of the label PNG; numbers above 65535 saturate (the table keeps every droplet)."""
    return np.minimum(np.asarray(labels), 65535).astype(np.uint16)
