"""A deliberately slow restatement of the droplet split ("Splitting touching droplets") in plain loops and dicts,
so that utils/droplet_split.py is not checked against itself.  The distance transform is scipy's
distance_transform_edt, squared and rounded (exact while the squared distance is far below 2^52)."""
import numpy as np
from scipy import ndimage

EDT_INF = 2 ** 31 - 1


def edt_sq_ref(mask):
    fg = np.asarray(mask) != 0
    if fg.all():
        return np.full(fg.shape, EDT_INF, np.int64)
    d = ndimage.distance_transform_edt(fg)
    return np.rint(d * d).astype(np.int64)


def passes(P, S, h2):
    """sqrt(P) - sqrt(S) <= h2 / 2 in Python integers."""
    t = 4 * P - 4 * S - h2 * h2
    return t <= 0 or t * t <= 16 * h2 * h2 * S


def split_ref(mask, h2, min_area=1):
    """-> (labels [h, w] int32, rows) with rows = [(area, sum_row, sum_col, first_index)] in label order."""
    fg = (np.asarray(mask) != 0).tolist()
    h, w = len(fg), len(fg[0])
    d2 = edt_sq_ref(mask).tolist()
    nbrs = ((-1, 0), (0, -1), (0, 1), (1, 0))
    ptr = {}
    for y in range(h):
        for x in range(w):
            if not fg[y][x]:
                continue
            best = (d2[y][x], -(y * w + x))
            for dy, dx in nbrs:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and fg[yy][xx]:
                    best = max(best, (d2[yy][xx], -(yy * w + xx)))
            ptr[y * w + x] = -best[1]
    root = {}
    for p in ptr:
        chain = []
        q = p
        while q not in root and ptr[q] != q:
            chain.append(q)
            q = ptr[q]
        r = root.get(q, q)
        for c in chain:
            root[c] = r
        root[q] = r
    parent = {p: p for p in ptr}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for y in range(h):
        for x in range(w):
            if not fg[y][x]:
                continue
            p = y * w + x
            for yy, xx in ((y, x + 1), (y + 1, x)):
                if yy < h and xx < w and fg[yy][xx]:
                    q = yy * w + xx
                    A, B = root[p], root[q]
                    if A == B or passes(min(d2[A // w][A % w], d2[B // w][B % w]), min(d2[y][x], d2[yy][xx]), h2):
                        a, b = find(p), find(q)
                        if a != b:
                            parent[max(a, b)] = min(a, b)
    classes = {}
    for p in sorted(ptr):
        classes.setdefault(find(p), []).append(p)
    labels = np.zeros((h, w), np.int32)
    rows = []
    for first in sorted(classes, key=lambda r: classes[r][0]):
        px = classes[first]
        if len(px) < max(min_area, 1):
            continue
        rows.append((len(px), sum(p // w for p in px), sum(p % w for p in px), px[0]))
        for p in px:
            labels[p // w, p % w] = len(rows)
    return labels, rows
