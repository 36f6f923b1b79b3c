"""The separation weight map of the border-weighted loss on the host: the definition of DESIGN.md section 19 on numpy / scipy.

For one mask (foreground where > 0.5), its 4-connected components, a radius R (integer, 1..64) and a background pixel x:

    D1(x)  the smallest squared Euclidean distance (an integer) to a foreground pixel with |dy| <= R and |dx| <= R; that
           pixel's component is L1
    D2(x)  the smallest such distance to a pixel of a component other than L1 (D2 = D1 when two components tie: the pair is
           unique even though L1 is not); EDT_INF where nothing qualifies.  Foreground pixels have D1 = D2 = 0.
    w(x) = 1 + w0 * exp(-(sqrt(D1) + sqrt(D2))^2 / (2 sigma^2))   on background pixels with D2 <= R^2, 1 everywhere else

Every pixel within Euclidean distance R lies inside the window, so {D2 <= R^2} and the distances there are those of the
untruncated transform: the map is the U-Net paper's separation term, set to zero where it is below w0 * exp(-R^2 / 2 sigma^2).

The planes are built in two passes, like the kernels of csrc/border.hip (which they equal bit for bit):

    column pass  per pixel, among the foreground pixels of its column with |dy| <= R: the nearest, (dy1, a), and the nearest
                 whose component differs from a, (dy2, b).  Two per column are enough: if the final L1 is not a, the column's
                 best pixel "other than L1" is the first candidate, otherwise the second.
    row pass     per pixel, over the columns |dx| <= R: (dx^2 + dy1^2, a) and (dx^2 + dy2^2, b) enter a running pair "best two
                 of distinct components" (insert()).

This module is the path of CPU tensors (``unet_dc_segmentation_amd.border.border_weights``) and the yardstick of the kernels;
tests/border_ref.py restates the definition as a brute-force window search and on scipy's distance transform per component.
"""
from __future__ import annotations

import math

import numpy as np

EDT_INF = 2 ** 31 - 1       # UNETDC_EDT_INF
MAX_SIDE = 16384
MAX_RADIUS = 64
DEFAULT_SIGMA = 5.0


def default_radius(sigma):
    """ceil(4 sigma), inside 1..MAX_RADIUS: the separation term is below w0 * exp(-8) beyond it."""
    return max(1, min(MAX_RADIUS, int(math.ceil(4.0 * float(sigma)))))


def check_params(w0, sigma, radius):
    """-> (w0, sigma, radius) as (float, float, int); ValueError for what unetdc_border_weights refuses."""
    w0, sigma = float(w0), float(sigma)
    if not (0.0 <= w0 < float("inf")) or not (0.0 < sigma < float("inf")):
        raise ValueError("border weights: w0 must be non-negative and sigma positive (both finite)")
    radius = default_radius(sigma) if radius is None else int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"border weights: the radius must be in 1..{MAX_RADIUS}, not {radius}")
    return w0, sigma, radius


def components(fg):
    """int64 [h, w]: a number unique per 4-connected component on foreground, -1 on background."""
    from scipy import ndimage
    lab = ndimage.label(fg)[0].astype(np.int64)            # default structure: 4-connectivity
    return lab - 1


def _shift(a, d, axis, fill):
    """b[i] = a[i + d] along `axis`, `fill` where i + d falls outside."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(d) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(d, 0), n + min(d, 0))
    dst[axis] = slice(max(-d, 0), n - max(d, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def insert(d, l, d1, l1, d2, l2):
    """The candidates (d, l) (l < 0: none) into the running best two of distinct components, in place, pixel by pixel:
    same component as the first: the minimum goes into the first; d < the first: the first moves to the second and the
    candidate becomes the first; same component as the second: the minimum into the second; d < the second: it replaces it."""
    ok = l >= 0
    c1 = ok & (l == l1)
    c2 = ok & ~c1 & (d < d1)
    c3 = ok & ~c1 & ~c2 & (l == l2)
    c4 = ok & ~c1 & ~c2 & ~c3 & (d < d2)
    nd1 = np.where(c1, np.minimum(d1, d), np.where(c2, d, d1))
    nl1 = np.where(c2, l, l1)
    nd2 = np.where(c2, d1, np.where(c3, np.minimum(d2, d), np.where(c4, d, d2)))
    nl2 = np.where(c2, l1, np.where(c4, l, l2))
    d1[...], l1[...], d2[...], l2[...] = nd1, nl1, nd2, nl2


def distance_planes(mask, radius):
    """(D1, D2) int32 [h, w] of one mask ([h, w], foreground where > 0.5)."""
    fg = np.asarray(mask) > 0.5
    if fg.ndim != 2 or not 1 <= fg.shape[0] <= MAX_SIDE or not 1 <= fg.shape[1] <= MAX_SIDE:
        raise ValueError("border weights: one [h, w] mask with sides 1..16384")
    R = int(radius)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"border weights: the radius must be in 1..{MAX_RADIUS}, not {radius}")
    lab = components(fg)
    shape = fg.shape
    new = lambda v: np.full(shape, v, np.int64)             # noqa: E731
    # column pass: by increasing |dy|, so the first foreground pixel met is the nearest, and the first of another component
    # the nearest of another component
    e1, a, e2, b = new(EDT_INF), new(-1), new(EDT_INF), new(-1)
    for dy in range(0, R + 1):
        for s in ((dy,) if dy == 0 else (-dy, dy)):
            v = _shift(lab, s, 0, -1)
            first = (v >= 0) & (a < 0)
            second = (v >= 0) & ~first & (v != a) & (b < 0)
            a[first], e1[first] = v[first], dy
            b[second], e2[second] = v[second], dy
    # row pass
    d1, l1, d2, l2 = new(EDT_INF), new(-1), new(EDT_INF), new(-1)
    for dx in range(-R, R + 1):
        sa, sb = _shift(a, dx, 1, -1), _shift(b, dx, 1, -1)
        s1, s2 = _shift(e1, dx, 1, 0), _shift(e2, dx, 1, 0)
        insert(dx * dx + s1 * s1, sa, d1, l1, d2, l2)
        insert(dx * dx + s2 * s2, sb, d1, l1, d2, l2)
    d1[fg] = 0
    d2[fg] = 0
    return d1.astype(np.int32), d2.astype(np.int32)


def weights_from_planes(d1, d2, w0, sigma, radius):
    """float32 [.., h, w]: the weight of the definition from the integer planes (fp64 arithmetic, rounded once)."""
    d1, d2 = np.asarray(d1, np.int64), np.asarray(d2, np.int64)
    on = (d1 > 0) & (d2 <= int(radius) ** 2)
    s = np.sqrt(np.where(on, d1, 0).astype(np.float64)) + np.sqrt(np.where(on, d2, 0).astype(np.float64))
    w = 1.0 + float(w0) * np.exp(-(s * s) / (2.0 * float(sigma) ** 2))
    return np.where(on, w, 1.0).astype(np.float32)


def border_weights_numpy(target, w0, sigma=DEFAULT_SIGMA, radius=None, planes=False):
    """target: [..., h, w] (any leading dimensions: every [h, w] plane is an image of its own) -> float32 weights of the same
    shape; with planes=True: (weights, D1, D2), the planes int32."""
    w0, sigma, radius = check_params(w0, sigma, radius)
    t = np.asarray(target)
    if t.ndim < 2:
        raise ValueError("border weights: the target needs at least two dimensions")
    flat = t.reshape((-1,) + t.shape[-2:])
    d1 = np.empty(flat.shape, np.int32)
    d2 = np.empty(flat.shape, np.int32)
    for i, m in enumerate(flat):
        d1[i], d2[i] = distance_planes(m, radius)
    w = weights_from_planes(d1, d2, w0, sigma, radius).reshape(t.shape)
    return (w, d1.reshape(t.shape), d2.reshape(t.shape)) if planes else w
