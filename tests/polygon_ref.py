"""Brute-force point-in-polygon fill for the polygon rasteriser's tests: Python integers, the inside
rule as the definition states it, one test per (pixel, polygon, edge).  It shares no code with utils/polygon_masks.py."""
import numpy as np


def quantise(v):
    """One float coordinate -> sub-pixels: v * 256 is exact in binary floating point, round() rounds half to even."""
    return int(round(float(v) * 256))


def inside(rings, X, Y):
    """rings: lists of (x, y) integer vertices of ONE polygon; (X, Y): the point, in the same units."""
    odd = False
    for ring in rings:
        n = len(ring)
        for i in range(n):
            (x0, y0), (x1, y1) = ring[i], ring[(i + 1) % n]
            if (y0 <= Y) == (y1 <= Y):
                continue
            if y0 > y1:
                x0, y0, x1, y1 = x1, y1, x0, y0
            if (X - x0) * (y1 - y0) > (Y - y0) * (x1 - x0):
                odd = not odd
    return odd


def fill(features, h, w):
    """features: [{"label": k, "polygons": [[ring, ...], ...]}] with float vertices -> int64 [h, w]: the largest label among the
    polygons whose inside holds the pixel's centre (256 c + 128, 256 r + 128)."""
    out = np.zeros((h, w), np.int64)
    for f in features:
        for poly in f["polygons"]:
            q = [[(quantise(x), quantise(y)) for x, y in ring] for ring in poly]
            for r in range(h):
                for c in range(w):
                    if f["label"] > out[r, c] and inside(q, 256 * c + 128, 256 * r + 128):
                        out[r, c] = f["label"]
    return out
