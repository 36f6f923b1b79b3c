"""The separation weight map of DESIGN.md section 19, restated for the tests independently of utils/border_weights.py (no column
pass, no candidate pair): a brute-force search of the (2R + 1)^2 window around every pixel, and scipy's Euclidean distance
transform taken once per component and sorted.  Also the masks of the edge cases both GPU and CPU tests walk through."""
import numpy as np

INF = 2 ** 31 - 1


def labels4(fg):
    """int [h, w]: 1.. per 4-connected component by flood fill, 0 on background."""
    h, w = fg.shape
    lab = np.zeros((h, w), np.int64)
    nxt = 0
    for y0 in range(h):
        for x0 in range(w):
            if not fg[y0, x0] or lab[y0, x0]:
                continue
            nxt += 1
            lab[y0, x0] = nxt
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < h and 0 <= xx < w and fg[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = nxt
                        stack.append((yy, xx))
    return lab


def brute_planes(mask, R):
    """(D1, D2) int32 by the definition: per background pixel, per component the smallest squared distance over the window;
    D1 the smallest of those, D2 the second smallest (of ANOTHER component: equal to D1 on a tie)."""
    fg = np.asarray(mask) > 0.5
    h, w = fg.shape
    lab = labels4(fg)
    pad = np.zeros((h + 2 * R, w + 2 * R), np.int32)
    pad[R:R + h, R:R + w] = lab
    dxs = np.arange(-R, R + 1, dtype=np.int32) ** 2
    dys = [dy for dy in range(-R, R + 1) if abs(dy) < h]    # a row offset of h or more meets no pixel of the image
    inf = np.int32(INF)

    def rows(dy):
        """(labels [h, w, 2R + 1] at (y + dy, x - R .. x + R), 0 outside the image; their squared distances [2R + 1])"""
        return np.lib.stride_tricks.sliding_window_view(pad[R + dy:R + dy + h], 2 * R + 1, axis=1), dy * dy + dxs

    # sweep 1: the nearest foreground pixel of the window
    d1 = np.full((h, w), inf, np.int32)
    for dy in dys:
        v, d = rows(dy)
        np.minimum(d1, np.where(v > 0, d, inf).min(axis=2), out=d1)
    # sweep 2: L1, a component met at exactly that distance (the smallest number among them)
    l1 = np.full((h, w), inf, np.int32)
    for dy in dys:
        v, d = rows(dy)
        np.minimum(l1, np.where((v > 0) & (d == d1[:, :, None]), v, inf).min(axis=2), out=l1)
    # sweep 3: the nearest pixel of a component other than L1 (another component tied for nearest is found at D1 itself)
    d2 = np.full((h, w), inf, np.int32)
    for dy in dys:
        v, d = rows(dy)
        np.minimum(d2, np.where((v > 0) & (v != l1[:, :, None]), d, inf).min(axis=2), out=d2)
    d2 = np.where(d1 == INF, INF, d2)
    d1[fg] = 0
    d2[fg] = 0
    return d1.astype(np.int32), d2.astype(np.int32)


def scipy_planes(mask):
    """(D1, D2) int64 of the UNTRUNCATED transform: the squared distance to every component by scipy's feature transform
    (integer offsets to a true nearest pixel), the two smallest per pixel; INF where fewer components exist; 0 on foreground."""
    from scipy import ndimage
    fg = np.asarray(mask) > 0.5
    h, w = fg.shape
    lab = labels4(fg)
    yy, xx = np.mgrid[0:h, 0:w]
    d1 = np.full((h, w), INF, np.int64)
    d2 = np.full((h, w), INF, np.int64)
    for l in range(1, int(lab.max()) + 1):
        idx = ndimage.distance_transform_edt(lab != l, return_distances=False, return_indices=True)
        d = (idx[0].astype(np.int64) - yy) ** 2 + (idx[1].astype(np.int64) - xx) ** 2
        d2 = np.minimum(d2, np.maximum(d1, d))
        d1 = np.minimum(d1, d)
    d1[fg] = 0
    d2[fg] = 0
    return d1, d2


def weight64(d1, d2, w0, sigma, R):
    """(on, term) in fp64 from integer planes: the pixels that carry a border term and the term there (0 elsewhere)."""
    d1, d2 = np.asarray(d1, np.int64), np.asarray(d2, np.int64)
    on = (d1 > 0) & (d2 <= R * R)
    s = np.sqrt(np.where(on, d1, 0).astype(np.float64)) + np.sqrt(np.where(on, d2, 0).astype(np.float64))
    return on, np.where(on, float(w0) * np.exp(-(s * s) / (2.0 * float(sigma) ** 2)), 0.0)


def term_bound(R, sigma):
    """Relative error allowed on the border term in fp32: a handful of roundings in an exponent of at most 2 R^2 / sigma^2,
    plus expf."""
    return (8.0 * 2.0 * R * R / (sigma * sigma) + 4.0) * 2.0 ** -24


def noise_mask(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.float32)


def edge_cases(R):
    """[(name, mask float32 [h, w])]: the smallest masks that can go wrong at radius R."""
    z = lambda h, w: np.zeros((h, w), np.float32)           # noqa: E731
    out = []
    for h, w in ((1, 1), (1, 9), (9, 1)):
        out.append((f"empty_{h}x{w}", z(h, w)))
        out.append((f"full_{h}x{w}", z(h, w) + 1))
        m = z(h, w)
        m[0, 0] = 1
        out.append((f"one_pixel_{h}x{w}", m))
    m = z(1, 9); m[0, 2] = m[0, 4] = 1                      # noqa: E702
    out.append(("two_pixels_gap_row", m))
    m = z(9, 1); m[2, 0] = m[4, 0] = 1                      # noqa: E702
    out.append(("two_pixels_gap_column", m))
    m = z(7, 9); m[2:5, 3:6] = 1                            # noqa: E702
    out.append(("one_droplet", m))
    m = z(6, 7); m[2, 3] = m[3, 4] = 1                      # noqa: E702
    out.append(("diagonal_neighbours", m))
    # B directly behind A in the column of the probe pixels below them, nothing else in reach
    m = z(2 * R + 12, 5); m[3, 2] = 1; m[1, 2] = 1          # noqa: E702
    out.append(("behind_in_column", m))
    # a U around background: its other arm is the same component
    m = z(9, 9); m[1:7, 2] = 1; m[1:7, 6] = 1; m[6, 2:7] = 1   # noqa: E702
    out.append(("u_shape", m))
    m2 = m.copy(); m2[0, 4] = 1                             # noqa: E702
    out.append(("u_shape_and_pixel", m2))
    # second droplet at squared distance exactly R^2 from the probe (row 2, column 1), and at R^2 + 1 (still inside the window)
    for extra, name in ((0, "second_at_R"), (1, "second_past_R")):
        m = z(5, R + 6); m[2, 0] = 1; m[2 + extra, 1 + R] = 1   # noqa: E702
        out.append((name, m))
    m = z(8, 11); m[0, 0] = m[0, 10] = m[7, 0] = m[7, 10] = 1; m[3:5, 0] = 1; m[0, 4:7] = 1   # noqa: E702
    out.append(("borders_and_corners", m))
    return out
