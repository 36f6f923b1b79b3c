"""Plain-loop restatement of DESIGN.md section 24, written from the definition alone: all four corners of all pixels of a
label, a textbook monotone chain over them, brute-force calipers with Python integers.  Shares no code with
utils/droplet_hull.py or csrc/hull.hip."""
import numpy as np

QUANTITIES = ("H2", "F2", "Wc", "Wl", "nv")


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """Andrew's monotone chain over (x, y) integer points -> the vertices in counter-clockwise order of the (x, y) plane,
    without collinear points."""
    pts = sorted(set(points))
    if len(pts) <= 2:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def corners(pixels):
    """[(y, x), ...] -> the corner points (x, y) of the pixels' unit squares."""
    out = []
    for y, x in pixels:
        out += [(x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)]
    return out


def hull_integers(pixels):
    """The pixels [(y, x), ...] of one label (at least one) -> (H2, F2, Wc, Wl, nv)."""
    v = convex_hull(corners(pixels))
    n = len(v)
    h2 = 0
    for i in range(n):
        a, b = v[i], v[(i + 1) % n]
        h2 += a[0] * b[1] - b[0] * a[1]
    h2 = abs(h2)
    f2 = 0
    for a in v:
        for b in v:
            f2 = max(f2, (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)
    best = None
    for i in range(n):
        p, q = v[i], v[(i + 1) % n]
        wc = max(abs(cross(p, q, u)) for u in v)
        wl = (q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2
        # the smallest Wc^2 / Wl by cross-multiplication, then the smallest Wl
        if best is None or wc * wc * best[1] < best[0] * best[0] * wl or (wc * wc * best[1] == best[0] * best[0] * wl and wl < best[1]):
            best = (wc, wl)
    return h2, f2, best[0], best[1], n


def label_hull_ref(labels, max_out):
    """labels: int [h, w] -> dict of int64 arrays [max_out] under QUANTITIES: 0 everywhere for a label without pixels; labels
    outside 1..max_out are skipped."""
    lab = np.asarray(labels)
    pixels = {}
    for y in range(lab.shape[0]):
        for x in range(lab.shape[1]):
            k = int(lab[y, x])
            if 1 <= k <= max_out:
                pixels.setdefault(k, []).append((y, x))
    out = {q: np.zeros(max_out, np.int64) for q in QUANTITIES}
    for k, px in pixels.items():
        for q, val in zip(QUANTITIES, hull_integers(px)):
            out[q][k - 1] = val
    return out


def hull_corner_points(labels, k):
    """The corner points (x, y) of label k, for a cross-check against another hull code."""
    ys, xs = np.nonzero(np.asarray(labels) == k)
    return corners(list(zip(ys.tolist(), xs.tolist())))
