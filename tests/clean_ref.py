"""Plain-loop restatement of the mask-cleaning stage, written from DESIGN.md section 13 alone (breadth-first fill, no scipy),
and the named small cases the CPU and GPU tests share.  Slow on purpose: small masks only."""
from collections import deque

import numpy as np


def components(on):
    """4-connected components of the True cells of a list-of-lists grid: a list of pixel lists [(y, x), ...]."""
    h, w = len(on), len(on[0])
    seen = [[False] * w for _ in range(h)]
    out = []
    for y0 in range(h):
        for x0 in range(w):
            if not on[y0][x0] or seen[y0][x0]:
                continue
            seen[y0][x0] = True
            comp, queue = [], deque([(y0, x0)])
            while queue:
                y, x = queue.popleft()
                comp.append((y, x))
                for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= ny < h and 0 <= nx < w and on[ny][nx] and not seen[ny][nx]:
                        seen[ny][nx] = True
                        queue.append((ny, nx))
            out.append(comp)
    return out


def clean_ref(strong, weak=None, max_hole_area=0):
    """-> (uint8 mask, [added, holes filled, pixels filled, holes left open]) by the three steps of section 13."""
    strong = np.asarray(strong)
    h, w = strong.shape
    S = [[bool(strong[y, x]) for x in range(w)] for y in range(h)]
    added = filled = pixels = left = 0
    if weak is None:
        M = [row[:] for row in S]
    else:
        weak = np.asarray(weak)
        W = [[bool(weak[y, x]) for x in range(w)] for y in range(h)]
        M = [[False] * w for _ in range(h)]
        for comp in components(W):
            if any(S[y][x] for y, x in comp):         # a pixel of the component where strong is 1 as well
                for y, x in comp:
                    M[y][x] = True
        for y in range(h):
            for x in range(w):
                added += M[y][x] and not S[y][x]
    if max_hole_area != 0:
        for comp in components([[not v for v in row] for row in M]):
            if any(y == 0 or y == h - 1 or x == 0 or x == w - 1 for y, x in comp):
                continue                              # reaches the first or last row or column: not a hole
            if max_hole_area < 0 or len(comp) <= max_hole_area:
                filled += 1
                pixels += len(comp)
                for y, x in comp:
                    M[y][x] = True
            else:
                left += 1
    return np.array(M, dtype=np.uint8), [int(added), filled, pixels, left]


def spiral(n):
    """A one-pixel-wide line spiralling inwards from (0, 0), one pixel of background between its arms."""
    m = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        moved = False
        while True:
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                break
            y, x, moved = ny, nx, True
            m[y, x] = 1
        if not moved:
            return m
        dy, dx = dx, -dy


def noise(h, w, seed, p=0.5):
    return (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)


def _grid(rows):
    return np.array([[int(c != ".") for c in r] for r in rows], np.uint8)


def named_cases():
    """name -> (strong, weak or None, max_hole_area)."""
    c = {}
    c["1x1_bg"] = (np.zeros((1, 1), np.uint8), None, -1)
    c["1x1_fg"] = (np.ones((1, 1), np.uint8), np.ones((1, 1), np.uint8), -1)
    c["1x7"] = (_grid(["#.#..#."]), _grid(["###.##."]), -1)
    c["7x1"] = (_grid(["#.#..#."]).T.copy(), _grid(["###.##."]).T.copy(), -1)
    c["all_zero"] = (np.zeros((6, 9), np.uint8), np.zeros((6, 9), np.uint8), -1)
    c["all_one"] = (np.ones((6, 9), np.uint8), np.ones((6, 9), np.uint8), -1)
    c["hole_3x3"] = (_grid(["###", "#.#", "###"]), None, -1)
    c["hole_open_to_border"] = (_grid(["#####", "#...#", "#.###", "#.#.#", "#.###"]), None, -1)     # leaves through (4, 1); (3, 3) is a hole
    c["diamond_ring"] = (_grid([".##.", "#..#", "#..#", ".##."]), None, -1)
    ring = np.zeros((11, 12), np.uint8)
    ring[1:10, 1:11] = 1
    ring[2:9, 2:10] = 0
    ring[4:7, 4:8] = 1                                # a droplet inside the hole
    ring[5, 5] = 0                                    # with a hole of its own
    c["droplet_in_hole_in_ring"] = (ring, None, -1)
    two = np.zeros((7, 14), np.uint8)
    two[1:6, 1:13] = 1
    two[2:4, 2:4] = 0                                 # area 4 = N
    two[2:4, 6:8] = 0
    two[4, 6] = 0                                     # area 5 = N + 1
    c["holes_N_and_N_plus_1"] = (two, None, 4)
    w_last = _grid([".....", ".###.", ".#...", ".##..", "....."])
    s_last = np.zeros_like(w_last)
    s_last[3, 2] = 1                                  # the component's last pixel in raster order
    c["seed_is_last_pixel"] = (s_last, w_last, 0)
    c["weak_without_strong"] = (np.zeros((5, 6), np.uint8), _grid(["......", ".##...", ".##.#.", "....#.", "......"]), 0)
    w_diag = _grid(["##...", "##...", "..##.", "..##.", "....."])
    s_diag = np.zeros_like(w_diag)
    s_diag[0, 0] = 1
    c["diagonal_weak_components"] = (s_diag, w_diag, 0)
    w_out = _grid(["......", ".###..", "......", "......"])
    s_out = _grid(["......", "..#...", "......", "....#."])      # (3, 4) is strong but not weak
    c["strong_outside_weak"] = (s_out, w_out, 0)
    eq = noise(9, 11, 5, 0.6)
    c["weak_equals_strong"] = (eq, eq.copy(), 0)
    sp = spiral(64)
    tip = np.zeros_like(sp)
    ys, xs = np.nonzero(sp)
    k = int(np.argmax((np.abs(ys - 32) + np.abs(xs - 32)) * -1))          # a pixel near the centre: far along the line
    tip[ys[k], xs[k]] = 1
    c["spiral_foreground"] = (tip, sp, -1)
    c["spiral_background"] = ((1 - sp).astype(np.uint8), None, -1)
    nz = noise(37, 83, 7, 0.55)
    c["noise_37x83"] = ((nz & noise(37, 83, 8, 0.3)).astype(np.uint8), nz, 3)
    return c


def weak_for(strong, seed=0):
    """A weak mask for the cases that have none: strong plus noise, so that strong is a subset of it."""
    return (strong | noise(strong.shape[0], strong.shape[1], 1000 + seed, 0.35)).astype(np.uint8)
