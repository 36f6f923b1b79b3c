"""Plain-loop restatement of DESIGN.md section 26 (Ripley's K of droplet centroids with simulated patterns), written from the
definition alone: Python integers, lists and loops, no numpy in the arithmetic.  tests/test_spatial_cpu.py pins
utils/spatial_stats.py to it, integer for integer; the hand fixtures with known answers live here too."""
import numpy as np

INF = 2 ** 31 - 1
M32 = 0xFFFFFFFF


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def hash_u(seed, s, k):
    rowkey = fmix32(fmix32(seed) ^ ((s * 0x9E3779B9) & M32))
    hi = fmix32(rowkey ^ (2 * k))
    lo = fmix32(rowkey ^ (2 * k + 1))
    return hi * 2 ** 32 + lo


def window_pixels(window, h, w):
    """The pixels of the window in raster order."""
    return [(y, x) for y in range(h) for x in range(w) if window is None or window[y][x]]


def points_of_table(area, sy, sx, h, w, window=None):
    """-> (points in table order, n_dropped)"""
    pts, dropped = [], 0
    for a, s0, s1 in zip(area, sy, sx):
        a, s0, s1 = int(a), int(s0), int(s1)
        y, x = (2 * s0 + a) // (2 * a), (2 * s1 + a) // (2 * a)
        if 0 <= y < h and 0 <= x < w and (window is None or window[y][x]):
            pts.append((y, x))
        else:
            dropped += 1
    return pts, dropped


def border_radius(p, h, w, R, zeros):
    """e(p); zeros: the zero pixels of the window inside the image (none: D2_W is infinite)."""
    y, x = p
    m = min(y + 1, x + 1, h - y, w - x)
    b2 = min(INF, m * m)
    for qy, qx in zeros:
        b2 = min(b2, (qy - y) ** 2 + (qx - x) ** 2)
    e = 0
    for r in range(R + 1):
        if r * r < b2:
            e = r
    return e


def pair_radius(p, q):
    d2 = (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2
    c = 0
    while c * c < d2:
        c += 1
    return c


def set_counts(pts, h, w, R, zeros):
    n, pairs, pairs_all = [0] * (R + 1), [0] * (R + 1), [0] * (R + 1)
    es = [border_radius(p, h, w, R, zeros) for p in pts]
    for r in range(R + 1):
        n[r] = sum(1 for e in es if e >= r)
    for i, p in enumerate(pts):
        for j, q in enumerate(pts):
            if i == j or abs(p[0] - q[0]) > R or abs(p[1] - q[1]) > R:
                continue
            c = pair_radius(p, q)
            for r in range(c, R + 1):
                pairs_all[r] += 1
                if es[i] >= r:
                    pairs[r] += 1
    return n, pairs, pairs_all


def simulated(seed, s, N, inside):
    A = len(inside)
    return [inside[(hash_u(seed, s, k) * A) >> 64] for k in range(N)]


def ripley_counts(pts, h, w, R, S, seed, window=None):
    """-> (n, pairs, pairs_all), lists of 1 + S rows of R + 1 integers"""
    win = None if window is None else [[int(v) for v in row] for row in np.asarray(window).tolist()]
    inside = window_pixels(win, h, w)
    zeros = [] if win is None else [(y, x) for y in range(h) for x in range(w) if not win[y][x]]
    rows = [set_counts(list(pts), h, w, R, zeros)]
    for s in range(S):
        if len(pts) == 0 or len(inside) == 0:
            rows.append(([0] * (R + 1),) * 3)
        else:
            rows.append(set_counts(simulated(seed, s, len(pts), inside), h, w, R, zeros))
    return tuple([list(r[q]) for r in rows] for q in range(3))


def hand_fixtures():
    """{name: (points, h, w, R, window or None, checks)}; checks: {"c": the pair radius of points 0 and 1, "e": [e per point],
    "pairs_all": {r: count}, "dropped": n} as far as the case fixes them."""
    f = {}
    f["offset_3_4"] = ([(10, 10), (13, 14)], 40, 40, 8, None, {"c": 5, "pairs_all": {4: 0, 5: 2, 8: 2}, "e": [8, 8]})
    f["offset_4_4"] = ([(10, 10), (14, 14)], 40, 40, 8, None, {"c": 6, "pairs_all": {5: 0, 6: 2}})
    f["coincident"] = ([(7, 9), (7, 9)], 30, 30, 3, None, {"c": 0, "pairs_all": {0: 2, 3: 2}})
    f["one_point"] = ([(5, 5)], 11, 11, 4, None, {"pairs_all": {0: 0, 4: 0}, "e": [4]})
    f["no_point"] = ([], 9, 9, 4, None, {"pairs_all": {0: 0, 4: 0}})
    f["corner"] = ([(0, 0), (8, 12), (4, 6)], 9, 13, 5, None, {"e": [0, 0, 4]})
    f["square_b2"] = ([(3, 20), (20, 8)], 41, 41, 16, None, {"e": [3, 8]})         # m = 4 -> e = 3; m = 9 -> e = 8
    hole = np.ones((21, 21), np.uint8)
    hole[10, 11] = 0
    f["hole_next_to_point"] = ([(10, 10), (10, 14)], 21, 21, 6, hole, {"e": [0, 2]})   # D2 = 1 -> e = 0; D2 = 9 -> e = 2
    f["all_ones_window"] = ([(10, 10), (13, 14), (2, 2)], 21, 21, 6, np.ones((21, 21), np.uint8), {"e": [6, 6, 2]})
    one = np.zeros((7, 9), np.uint8)
    one[3, 4] = 1
    f["one_pixel_window"] = ([(3, 4), (3, 4), (3, 4)], 7, 9, 3, one, {"c": 0, "e": [0, 0, 0], "pairs_all": {0: 6}})
    return f


def random_case(h, w, N, window_kind, seed):
    """(area, sy, sx, window): a droplet table of N droplets with areas 1..40 whose centroids fall anywhere in the image, some on
    the frame, two on one pixel; window_kind: "null", "noisy" (a tenth of the pixels outside) or "holes"."""
    rng = np.random.default_rng(seed)
    area = rng.integers(1, 41, N)
    y, x = rng.integers(0, h, N), rng.integers(0, w, N)
    if N >= 4:
        y[0], x[0], y[1], x[1] = 0, 0, h - 1, w - 1
        y[3], x[3] = y[2], x[2]
    sy, sx = y * area + rng.integers(0, area) // 2, x * area + rng.integers(0, area) // 2     # below half a pixel up
    window = None
    if window_kind == "noisy":
        window = (rng.random((h, w)) >= 0.1).astype(np.uint8)
        window[y[-1], x[-1]] = 0                               # at least one droplet is dropped
    elif window_kind == "holes":
        window = np.ones((h, w), np.uint8)
        window[h // 3:h // 3 + 5, w // 4:w // 4 + 9] = 0
        window[h - 4:, :7] = 0
        window[0, w - 1] = 0
        window[:, 64:66] = np.where(np.arange(h)[:, None] % 3 == 0, 0, 1)
    return area.astype(np.int64), sy.astype(np.int64), sx.astype(np.int64), window
