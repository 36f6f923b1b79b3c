"""Cases shared by tests/test_polygons_cpu.py and tests/test_gpu_polygons.py: the seeded random polygons
with their brute-force answers (computed once), the known answers written out by hand from the rule, and the label maps of the
round trips."""
import functools

import numpy as np

from tests import polygon_ref
from tests.test_outlines_cpu import fill_mask, known_map, known_shapes, minus

N_RANDOM = 200


def feature(label, *polygons):
    """polygons: each a list of rings, each ring a list of (x, y)."""
    return {"label": label, "polygons": [[np.asarray(r, dtype=np.float64) for r in poly] for poly in polygons]}


def random_case(t):
    """Case t -> (features, h, w): sides 1..12, one polygon of 1-2 rings of 3-8 vertices in [-3, side + 3]; every third case on
    multiples of 0.5, where pixel centres lie on edges and vertices."""
    rng = np.random.default_rng(2800 + t)
    h, w = (int(v) for v in rng.integers(1, 13, size=2))
    rings = []
    for _ in range(int(rng.integers(1, 3))):
        n = int(rng.integers(3, 9))
        if t % 3 == 0:
            pts = np.stack((rng.integers(-6, 2 * (w + 3) + 1, size=n), rng.integers(-6, 2 * (h + 3) + 1, size=n)), axis=1) / 2.0
        else:
            pts = np.stack((rng.uniform(-3, w + 3, size=n), rng.uniform(-3, h + 3, size=n)), axis=1)
        rings.append(pts)
    return [feature(int(rng.integers(1, 6)), rings)], h, w


@functools.lru_cache(maxsize=None)
def random_answers():
    """The brute-force label maps of the N_RANDOM cases, computed once per process and never written to."""
    out = []
    for t in range(N_RANDOM):
        feats, h, w = random_case(t)
        a = polygon_ref.fill(feats, h, w)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1)]


def known_answers():
    """name -> (features, h, w, expected plane), the planes written out by hand from the inside rule.
    shifted: the centre of column 0 lies ON the left edge x = 0.5 and is not right of it; the centre of column 1 is right of
    the left edge and lies on the right edge x = 1.5, which then does not count: one crossing, inside.
    vertex: the triangle (0.5, 0.5) (2.5, 0.5) (0.5, 2.5).  Its top edge is horizontal and never counts.  Row 0 (Y = 0.5) is
    crossed by the left edge x = 0.5 and by the hypotenuse at x = 2.5: centre 0 lies on the left edge (0 crossings), centres 1
    and 2 are right of the left edge and not right of the hypotenuse (centre 2 lies on it): inside.  Row 1 crosses the hypotenuse
    at x = 1.5: centre 1 lies on it (1 crossing, inside), centre 2 is right of both (outside).  Row 2 (Y = 2.5) has
    y1 <= Y for both edges: no crossing."""
    shift = [(x + 0.5, y) for x, y in SQUARE]
    return {
        "unit square": ([feature(1, [SQUARE])], 2, 3, [[1, 0, 0], [0, 0, 0]]),
        "shifted": ([feature(1, [shift])], 2, 3, [[0, 1, 0], [0, 0, 0]]),
        "shifted, one column": ([feature(1, [shift])], 2, 1, [[0], [0]]),
        "vertex": ([feature(4, [[(0.5, 0.5), (2.5, 0.5), (0.5, 2.5)]])], 3, 3, [[0, 4, 4], [0, 4, 0], [0, 0, 0]]),
        "no centre": ([feature(1, [[(0.1, 0.1), (0.4, 0.1), (0.1, 0.4)]])], 2, 2, [[0, 0], [0, 0]]),
    }


def round_trip_maps():
    """name -> label map: the cases whose outlines must fill back to the map."""
    island = minus(7, 7, *[(r, c) for r in range(1, 6) for c in range(1, 6)])
    island[3, 3] = 1                                          # an island in its own hole: a MultiPolygon
    out = {"known map": known_map(), "square minus centre": known_shapes()["square minus centre"][0],
           "ring with a core": known_shapes()["ring with a core"][0], "island in its hole": island,
           "diagonal hole": known_shapes()["diagonal hole"][0]}
    for t in range(6):
        out[f"mask {t}"] = fill_mask(24, 31, 2000 + t)
    return out
