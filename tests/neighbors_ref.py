"""The definition of DESIGN.md section 20 restated as plainly as possible: the smallest squared distance over ALL pixel pairs
of two labels, and a plain union-find over the contact pairs.  Shares no code with utils/droplet_neighbors.py or the
kernels.  Also the hand fixtures and label maps that tests/test_neighbors_cpu.py and tests/test_gpu_neighbors.py share."""
import functools

import numpy as np

INF = 2 ** 31 - 1


def brute_pairs(label, max_label, G):
    """-> [(a, b, d2)] in (a, b) order: every pixel of a against every pixel of b."""
    lab = np.asarray(label).astype(np.int64)
    pts = {}
    for k in range(1, int(max_label) + 1):
        ys, xs = np.nonzero(lab == k)
        if ys.size:
            pts[k] = (ys, xs)
    keys, out = sorted(pts), []
    for i, a in enumerate(keys):
        ya, xa = pts[a]
        for b in keys[i + 1:]:
            yb, xb = pts[b]
            if (yb.min() - ya.max() > G or ya.min() - yb.max() > G or xb.min() - xa.max() > G or xa.min() - xb.max() > G):
                continue                                          # bounding boxes further apart than G: no pixel pair can qualify
            d = ((ya[:, None] - yb[None, :]) ** 2 + (xa[:, None] - xb[None, :]) ** 2).min()
            if d <= G * G:
                out.append((a, b, int(d)))
    return out


def brute_columns(label, max_label, pairs):
    """-> {nn_label, nn_d2, degree, cluster, cluster_size}: lists of max_label ints, from the pair list by plain loops."""
    K = int(max_label)
    lab = np.asarray(label)
    present = [bool((lab == k).any()) for k in range(1, K + 1)]
    nn = [(INF, 0)] * K
    degree = [0] * K
    parent = list(range(K + 1))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b, d in pairs:
        degree[a - 1] += 1
        degree[b - 1] += 1
        nn[a - 1] = min(nn[a - 1], (d, b))
        nn[b - 1] = min(nn[b - 1], (d, a))
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    cluster = [find(k) for k in range(1, K + 1)]
    size = [sum(1 for j in range(K) if cluster[j] == cluster[k] and present[j]) if present[k] else 0 for k in range(K)]
    return {"nn_label": [n[1] for n in nn], "nn_d2": [n[0] for n in nn], "degree": degree, "cluster": cluster, "cluster_size": size}


def pixels(h, w, *points):
    """An h x w int32 map with label k + 1 at points[k] = (y, x)."""
    m = np.zeros((h, w), np.int32)
    for k, (y, x) in enumerate(points):
        m[y, x] = k + 1
    return m


def ring():
    m = np.zeros((9, 9), np.int32)
    m[0, :] = m[8, :] = m[:, 0] = m[:, 8] = 1
    m[4, 4] = 2
    return m


def hand_fixtures():
    """name -> (label map, max_label, G, the expected pair list).  The answers are written out by hand; the tests also check
    them against brute_pairs."""
    return {
        "disc_not_square": (pixels(12, 12, (1, 1), (5, 5), (6, 1), (1, 7)), 4, 5, [(1, 3, 25), (2, 3, 17), (2, 4, 20)]),
        "exactly_G": (pixels(8, 9, (1, 2), (4, 6)), 2, 5, [(1, 2, 25)]),
        "just_past_G": (pixels(8, 9, (1, 2), (4, 6)), 2, 4, []),
        "behind_in_column": (pixels(8, 9, (0, 4), (3, 4), (6, 4)), 3, 6, [(1, 2, 9), (1, 3, 36), (2, 3, 9)]),
        "touching_G1": (pixels(3, 4, (0, 0), (0, 1), (1, 2)), 3, 1, [(1, 2, 1)]),
        "touching_G2": (pixels(3, 4, (0, 0), (0, 1), (1, 2)), 3, 2, [(1, 2, 1), (2, 3, 2)]),
        "chain_and_islands": (pixels(1, 40, *((0, x) for x in (0, 3, 6, 9, 20, 22, 39))), 7, 3,
                              [(1, 2, 9), (2, 3, 9), (3, 4, 9), (5, 6, 4)]),
        "ring_G3": (ring(), 2, 3, []),
        "ring_G4": (ring(), 2, 4, [(1, 2, 16)]),
    }


def edge_maps():
    """name -> (label map, max_label): the geometries and label ranges at the edge of the definition."""
    g = np.random.default_rng(11)
    row = np.zeros((1, 130), np.int32)
    row[0, [0, 3, 63, 64, 65, 127, 128, 129]] = np.arange(1, 9)
    messy = pixels(6, 9, (0, 0), (0, 2), (2, 2), (5, 8))
    messy[0, 1], messy[1, 2], messy[3, 3], messy[5, 7] = 9, -3, -2 ** 31, 2 ** 31 - 1      # out of range: background, never a partner
    full_labels = g.permutation(np.arange(1, 7 * 11 + 1, dtype=np.int32)).reshape(7, 11)   # every pixel its own label
    return {
        "1x1": (np.ones((1, 1), np.int32), 1),
        "1x1_empty": (np.zeros((1, 1), np.int32), 3),
        "1x130": (row, 8),
        "130x1": (np.ascontiguousarray(row.T), 8),
        "empty": (np.zeros((5, 70), np.int32), 4),
        "one_droplet_fills_the_image": (np.ones((9, 67), np.int32), 1),
        "max_label_0": (pixels(4, 5, (1, 1), (1, 3)), 0),
        "out_of_range_values": (messy, 4),
        "labels_above_max_label": (pixels(4, 9, (1, 1), (1, 3), (1, 5), (1, 7)), 2),
        "label_without_pixel": (pixels(4, 9, (1, 1), (1, 3)) * 2, 5),                      # labels 2 and 4 of 1..5 exist
        "every_pixel_a_label": (full_labels, 77),
    }


@functools.lru_cache(maxsize=None)
def random_map(h=70, w=150, density=0.45, seed=5):
    """ndimage.label of an opened random mask -> (int32 label map, number of components); read only."""
    from scipy import ndimage
    m = np.random.default_rng(seed).random((h, w)) < density
    lab, n = ndimage.label(ndimage.binary_opening(m))
    lab = lab.astype(np.int32)
    lab.setflags(write=False)
    return lab, int(n)


@functools.lru_cache(maxsize=None)
def touching_map(h=97, w=131, seed=3, cells=9):
    """A map without background: Voronoi-like cells of random labels, so most contacts are at d2 = 1."""
    g = np.random.default_rng(seed)
    lab = g.integers(1, 40, size=((h + cells - 1) // cells, (w + cells - 1) // cells)).astype(np.int32)
    lab = np.kron(lab, np.ones((cells, cells), np.int32))[:h, :w]
    lab = np.ascontiguousarray(lab)
    lab.setflags(write=False)
    return lab, 39


# (h, w, step, G, labels, pairs): lattices of single-pixel droplets whose pair lists pass one, two and four sort chunks of 4096
LATTICES = ((64, 65, 1, 1, 4160, 8191), (129, 129, 2, 2, 4225, 8320), (129, 129, 2, 3, 4225, 16512), (91, 91, 1, 2, 8281, 48778))
CAP_LATTICE = (1500, 1500, 2, 2, 562500, 1123500)              # past the 2048 x 256 grids of the per-label and per-pair kernels


@functools.lru_cache(maxsize=None)
def lattice_map(h, w, step, seed=1):
    """-> (int32 map, k): single-pixel droplets every `step` pixels from (0, 0), labelled by a seeded permutation of 1..k, so
    label order is unrelated to raster order.  The nearest neighbours of a droplet all lie `step` away: the smaller label
    decides nn_label."""
    lab = np.zeros((h, w), np.int32)
    rows, cols = len(range(0, h, step)), len(range(0, w, step))
    k = rows * cols
    lab[::step, ::step] = (1 + np.random.default_rng(seed).permutation(k)).astype(np.int32).reshape(rows, cols)
    lab.setflags(write=False)
    return lab, k


def offset_pairs(lab, k, G):
    """A map of single-pixel droplets -> int64 (a, b, d2) in (a, b) order: for every offset (dy, dx) of the half plane with
    dy^2 + dx^2 <= G^2 the pixel pairs (p, p + offset) with two different labels in 1..k, keyed (smaller, larger), the minimum
    per key.  Plain shifted views; shares nothing with utils/droplet_neighbors.py."""
    lab = np.asarray(lab).astype(np.int64)
    lab = np.where((lab >= 1) & (lab <= int(k)), lab, 0)
    h, w = lab.shape
    keys, dist = [], []
    for dy in range(0, G + 1):
        for dx in range(-G, G + 1):
            if (dy == 0 and dx <= 0) or dy * dy + dx * dx > G * G or dy >= h or abs(dx) >= w:
                continue
            p = lab[:h - dy, max(-dx, 0):w - max(dx, 0)]
            q = lab[dy:, max(dx, 0):w - max(-dx, 0)]
            hit = (p > 0) & (q > 0) & (p != q)
            lo, hi = np.minimum(p[hit], q[hit]), np.maximum(p[hit], q[hit])
            keys.append((lo << 32) | hi)
            dist.append(np.full(lo.size, dy * dy + dx * dx, np.int64))
    if not keys:
        return tuple(np.zeros(0, np.int64) for _ in range(3))
    keys, dist = np.concatenate(keys), np.concatenate(dist)
    uniq, inverse = np.unique(keys, return_inverse=True)
    d2 = np.full(uniq.size, INF, np.int64)
    np.minimum.at(d2, inverse, dist)
    return uniq >> 32, uniq & 0xFFFFFFFF, d2


PATCH_SIZES = ((1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 1), (1, 3))       # droplets per patch: rows x columns
PATCH_G = 2
PATCH_MISSING = 7                                                             # labels of 1..K without a pixel


@functools.lru_cache(maxsize=None)
def patch_map(h=512, w=520, seed=4):
    """-> (int32 map, K, cluster [K], cluster_size [K]) for radius PATCH_G: one step-2 lattice patch of a seeded choice of
    PATCH_SIZES in the corner of every 8 x 8 cell (a patch spans at most 5 x 5 pixels: 3 > G pixels between two patches), labels a
    seeded permutation of 1..K of which the last PATCH_MISSING stay unused.  A patch is one cluster: its root is its smallest
    label, its size the patch's droplets; a label without a pixel is its own cluster of size 0."""
    g = np.random.default_rng(seed)
    cells = [(y, x) for y in range(0, h - 7, 8) for x in range(0, w - 7, 8)]
    sizes = [PATCH_SIZES[i] for i in g.integers(0, len(PATCH_SIZES), len(cells))]
    K = sum(r * c for r, c in sizes) + PATCH_MISSING
    labels = (1 + g.permutation(K)).astype(np.int64)
    lab = np.zeros((h, w), np.int32)
    cluster, size = np.arange(1, K + 1, dtype=np.int64), np.zeros(K, np.int64)
    at = 0
    for (y, x), (r, c) in zip(cells, sizes):
        mine = labels[at:at + r * c]
        at += r * c
        lab[y:y + 2 * r:2, x:x + 2 * c:2] = mine.reshape(r, c)
        cluster[mine - 1] = mine.min()
        size[mine - 1] = r * c
    assert at == K - PATCH_MISSING
    for v in (lab, cluster, size):
        v.setflags(write=False)
    return lab, K, cluster, size
