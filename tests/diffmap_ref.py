"""Plain-loop restatement of the difference map and its regions, for tests/test_diffmap_cpu.py and
tests/test_gpu_diffmap.py: lists, an explicit stack, eight neighbours, no scipy.  And the fixtures both test files share."""
import functools

import numpy as np

COLOR_TABLE = {0: (0, 0, 0), 1: (0, 255, 0), 2: (255, 0, 0), 3: (255, 255, 0)}      # the issue's table, literally
EIGHT = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def class_plane_ref(pred, gt):
    return [[(1 if p else 0) + (2 if g else 0) for p, g in zip(pr, gr)] for pr, gr in zip(pred, gt)]


def colors_ref(c):
    return [[COLOR_TABLE[v] for v in row] for row in c]


def overlay_ref(image, c):
    return [[COLOR_TABLE[v] if v else tuple(px) for v, px in zip(crow, irow)] for crow, irow in zip(c, image)]


def regions_ref(pred, gt, min_area=1):
    """-> (image: 12 integers, rows: [(class, area, sumy, sumx, neighbors)] of the classes 1..3 with area >= min_area).  Regions
    are found in raster order of their first pixel, which is the order of the table."""
    c = class_plane_ref(pred, gt)
    h, w = len(c), len(c[0])
    seen = [[False] * w for _ in range(h)]
    image, rows = [0] * 12, []
    for y0 in range(h):
        for x0 in range(w):
            image[c[y0][x0]] += 1
            if seen[y0][x0]:
                continue
            k = c[y0][x0]
            area = sy = sx = bits = 0
            stack = [(y0, x0)]
            seen[y0][x0] = True
            while stack:
                y, x = stack.pop()
                area, sy, sx = area + 1, sy + y, sx + x
                for dy, dx in EIGHT:
                    yy, xx = y + dy, x + dx
                    if not (0 <= yy < h and 0 <= xx < w):
                        continue
                    if c[yy][xx] != k:
                        bits |= 1 << c[yy][xx]
                    elif not seen[yy][xx]:
                        seen[yy][xx] = True
                        stack.append((yy, xx))
            image[4 + k] += 1
            if area >= min_area:
                image[8 + k] += 1
                if k:
                    rows.append((k, area, sy, sx, bits))
    return image, rows


def record_as_ref(rec):
    """A record of utils.difference_map / evaluate.diff_regions_batch in the form regions_ref returns."""
    return ([int(v) for v in rec["image"]],
            list(zip(*(rec[k].tolist() for k in ("class", "area", "sumy", "sumx", "neighbors")))))


# ---- fixtures: (pred, gt) pairs of uint8 planes ------------------------------------------------------------------------
def from_classes(c):
    c = np.asarray(c, np.uint8)
    return np.ascontiguousarray(c & 1), np.ascontiguousarray(c >> 1)


def checkerboard(h, w, a, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return from_classes(np.where((yy + xx) % 2 == 0, a, b))


def anti_diagonal(h, w, k, ground):
    """A one-pixel line of class k from the top right towards the bottom left: held together by NE neighbours alone."""
    c = np.full((h, w), ground, np.uint8)
    n = min(h, w)
    c[np.arange(n), w - 1 - np.arange(n)] = k
    return from_classes(c)


def four_class_tiles(h=64, w=64):
    return from_classes(np.tile(np.array([[0, 1], [2, 3]], np.uint8), (h // 2, w // 2)))


def serpentine(h=300, w=401):
    """A one-pixel path of class 3 that runs along every fourth row and turns at alternate ends, class 0 between its turns; the
    first and last row and column stay class 0, so the background is ONE region."""
    c = np.zeros((h, w), np.uint8)
    rows = list(range(1, h - 1, 4))
    for j, y in enumerate(rows):
        c[y, 1:w - 1] = 3
        if j + 1 < len(rows):
            x = w - 2 if j % 2 == 0 else 1
            c[y:rows[j + 1] + 1, x] = 3
    return from_classes(c)


def shifted(m, dy, dx):
    out = np.zeros_like(m)
    h, w = m.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = m[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def realistic(h, w, kind, seed=3):
    """gt = noise_mask; pred = that mask moved by one pixel, dilated by one, or an unrelated mask."""
    from scipy import ndimage
    from tests.test_split_cpu import noise_mask
    gt = noise_mask(h, w, seed)
    if kind == "moved":
        pred = shifted(gt, 1, 1)
    elif kind == "dilated":
        pred = ndimage.binary_dilation(gt, structure=np.ones((3, 3), bool)).astype(np.uint8)
    else:
        pred = noise_mask(h, w, seed + 100)
    return pred, gt


SHAPES = [(1, 1), (1, 64), (64, 1), (2, 2), (37, 53), (96, 130), (300, 401)]
FULL = (1040, 1388)


@functools.lru_cache(maxsize=None)
def small_cases():
    """{name: (pred, gt)}: everything below full size."""
    rng = np.random.default_rng(7)
    cases = {}
    for h, w in SHAPES:
        cases[f"random/{h}x{w}"] = from_classes(rng.integers(0, 4, (h, w)))
    for h, w in [(2, 2), (37, 53), (96, 130)]:
        cases[f"checkerboard03/{h}x{w}"] = checkerboard(h, w, 0, 3)
        cases[f"checkerboard12/{h}x{w}"] = checkerboard(h, w, 1, 2)
    for a, b in [(0, 1), (2, 3), (3, 0)]:
        cases[f"crossing{a}{b}"] = from_classes([[a, b], [b, a]])
    for k in range(4):
        cases[f"anti_diagonal{k}"] = anti_diagonal(96, 130, k, (k + 1) % 4)
    cases["four_classes"] = four_class_tiles()
    cases["serpentine"] = serpentine()
    for k in (0, 3):
        cases[f"all{k}/37x53"] = from_classes(np.full((37, 53), k))
    for kind in ("moved", "dilated", "unrelated"):
        cases[f"realistic_{kind}/96x130"] = realistic(96, 130, kind)
    return cases


@functools.lru_cache(maxsize=None)
def full_case():
    return realistic(*FULL, "moved", seed=5)
