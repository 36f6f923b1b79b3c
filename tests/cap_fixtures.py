"""Inputs of the hull, Ripley, border and outline tests of tests/test_gpu_grid_caps.py, each with the premise that says what it is for: an
assert that fails when the fixture stops reaching the loop, the tile or the limit it was built to reach.  Host code only;
tests/test_droplet_edges_cpu.py runs every premise without a device."""
import functools

import numpy as np

from tests import droplet_edge_fixtures as fx
from utils import droplet_hull as dh
from utils import spatial_stats as ss

NH = len(dh.QUANTITIES)


def label_heights(lab, max_out):
    """{label: (first row, rows)} of the labels 1..max_out with pixels, from one pass over the labelled pixels."""
    h, w = lab.shape
    idx = np.flatnonzero((lab.ravel() > 0) & (lab.ravel() <= max_out))             # raster order: rows ascend
    lbl = lab.ravel()[idx]
    order = np.argsort(lbl, kind="stable")
    lbl, ys = lbl[order], (idx // w)[order]
    present, first = np.unique(lbl, return_index=True)
    last = np.append(first[1:], len(lbl)) - 1
    return {int(k): (int(ys[a]), int(ys[b] - ys[a] + 1)) for k, a, b in zip(present, first, last)}


def rows_needed(lab, max_out):
    """The sum over the labels 1..max_out with pixels of max_y - min_y + 1 (what unetdc_label_hull reports in *out_rows)."""
    return sum(n for _, n in label_heights(lab, max_out).values())


def slots_used(lab, max_out):
    """The candidate slots hull_fill_kernel has to fill: a label of height H has H + 1 corner levels."""
    return sum(n + 1 for _, n in label_heights(lab, max_out).values())


def rect_integers(a, b):
    """(H2, F2, Wc, Wl, nv) of an a x b rectangle, a > b: twice the area, the squared diagonal, and the narrowest width b as
    the cross product a * b over the long edge a (squared length a^2)."""
    assert a > b >= 1
    return 2 * a * b, a * a + b * b, a * b, a * a, 4


# ---- hull: sparse high label numbers -------------------------------------------------------------------------------------------

HULL_SPARSE_SHAPE = (96, 130)
HULL_SPARSE_MAX_OUT = 65536        # what mask_and_droplets passes at full size
_T = fx.HULL_LABELS_PER_TRIP
# (label index k = number - 1, first row, rows, the share of rows with pixels); k and k + 16 384 share a wave on consecutive trips
HULL_SPARSE_SPEC = (
    (5, 2, 90, 1.0), (5 + _T, 10, 20, 1.0),                  # more than 64 levels, then at most 64: LDS, then the register path
    (100, 30, 37, 1.0), (100 + _T, 1, 94, 1.0),              # the other order
    (200, 20, 70, 1.0), (200 + 2 * _T, 5, 63, 1.0),          # 200 + 16 384 has no pixels; 63 rows are 64 levels, the register path's most
    (300, 0, 96, 1.0), (300 + _T, 31, 64, 1.0),              # two LDS labels in a row: 97 levels, then 65 (the path's fewest)
    (5 + 3 * _T, 8, 80, 0.4),                                # the fourth trip: scattered rows, empty levels in between
    (HULL_SPARSE_MAX_OUT - 1, 93, 3, 1.0),                   # the last number of all, in the last rows
    (_T - 1, 50, 1, 1.0), (_T, 60, 5, 1.0),                  # the last label of the first trip, the first of the second
    (7 + 2 * _T, 3, 88, 0.7), (7 + 3 * _T, 40, 1, 1.0),      # 7 and 7 + 16 384 have no pixels
)


@functools.lru_cache(maxsize=None)
def hull_sparse_maps():
    """-> (compact, high, numbers): the same pixel sets numbered 1..n in the order of HULL_SPARSE_SPEC, and by the spec's numbers."""
    h, w = HULL_SPARSE_SHAPE
    compact = np.zeros((h, w), np.int32)
    rng = np.random.default_rng(24)
    for i, (k, y0, rows, share) in enumerate(HULL_SPARSE_SPEC):
        x0 = 1 + 9 * i                                       # a strip of its own, a background column between neighbours
        assert x0 + 8 < w and y0 + rows <= h
        for r in range(rows):
            if 0 < r < rows - 1 and rng.random() >= share:
                continue
            lo, hi = x0 + int(rng.integers(0, 4)), x0 + 4 + int(rng.integers(0, 4))
            compact[y0 + r, lo:hi + 1] = i + 1
    numbers = np.array([k + 1 for k, _, _, _ in HULL_SPARSE_SPEC], np.int32)
    high = np.where(compact > 0, numbers[np.maximum(compact, 1) - 1], 0).astype(np.int32)
    for v in (compact, high, numbers):
        v.setflags(write=False)
    return compact, high, numbers


def scatter_rows(ref, numbers, max_out):
    """The rows of the compactly numbered map at the high numbers; every other number keeps what hull_init_kernel wrote: zeros."""
    out = np.zeros((NH, max_out), np.int64)
    for j, q in enumerate(dh.QUANTITIES):
        out[j, numbers - 1] = ref[q]
    return out


def assert_hull_sparse_premise(high, max_out):
    """Four trips of the chain and caliper kernels, each with a label that has pixels; on one wave, on consecutive trips: a label
    of more than 64 levels then one of at most 64, the other order, two LDS labels of different length, and a label without
    pixels after one with; a second trip of hull_init_kernel."""
    T = fx.HULL_LABELS_PER_TRIP
    assert T == 16384 and max_out > 3 * T and NH * max_out > fx.HULL_WORDS_PER_TRIP
    assert int(high.max()) == max_out                        # the last number of all has pixels
    levels = {k - 1: n + 1 for k, (_, n) in label_heights(high, max_out).items()}       # by label index
    assert {k // T for k in levels} == {0, 1, 2, 3}
    pairs = [(levels.get(k), levels.get(k + T)) for k in range(max_out - T)]
    seen = {(a > 64, b > 64) for a, b in pairs if a and b}
    assert seen >= {(True, False), (False, True), (True, True)}
    assert any(a and a > 64 and b is None for a, b in pairs)                            # the later label has no pixels
    assert any(a is None and b for a, b in pairs)                                       # ... and the earlier one
    assert any(a > 64 and b > 64 and a != b for a, b in pairs if a and b)               # stale LDS levels beyond the later label's
    assert 64 in levels.values() and 65 in levels.values()                              # both sides of the register path's limit
    assert max(levels.values()) <= fx.HULL_LDS_POINTS


# ---- hull: more used slots than one trip of hull_fill_kernel ------------------------------------------------------------------

HULL_COLUMNS_SHAPE = (2100, 130)
HULL_COLUMNS = 128
HULL_COLUMNS_SCATTERED = 4         # the last labels: a pixel on every 70th row and on the last


@functools.lru_cache(maxsize=None)
def hull_columns_map():
    """128 columns one pixel wide over the full height, label k in column k; the last four hold a pixel on every 70th row and
    on the last row only: their segments, beyond slot 262 144, are mostly levels without a candidate."""
    h, w = HULL_COLUMNS_SHAPE
    lab = np.zeros((h, w), np.int32)
    for k in range(1, HULL_COLUMNS + 1):
        if k <= HULL_COLUMNS - HULL_COLUMNS_SCATTERED:
            lab[:, k] = k
        else:
            lab[::70, k] = k
            lab[h - 1, k] = k
    lab.setflags(write=False)
    return lab


def assert_hull_columns_premise(lab):
    h, w = lab.shape
    heights = label_heights(lab, HULL_COLUMNS)
    assert len(heights) == HULL_COLUMNS and all(v == (0, h) for v in heights.values())
    assert h + 1 > fx.HULL_LDS_POINTS                        # the first chain pass runs in memory: it reads every level
    used = slots_used(lab, HULL_COLUMNS)
    assert used == HULL_COLUMNS * (h + 1) > fx.HULL_WORDS_PER_TRIP
    first_scattered = HULL_COLUMNS - HULL_COLUMNS_SCATTERED                              # label index
    assert first_scattered * (h + 1) < fx.HULL_WORDS_PER_TRIP < (first_scattered + 1) * (h + 1)   # its segment holds the boundary
    for k in range(first_scattered + 1, HULL_COLUMNS + 1):
        rows = np.flatnonzero(lab[:, k] == k)
        empty_levels = (h + 1) - len(np.union1d(rows, rows + 1))
        assert empty_levels > 0.9 * (h + 1) and (lab == k).sum() == len(rows)
    assert rows_needed(lab, HULL_COLUMNS) == HULL_COLUMNS * h


# ---- hull: coordinate limits ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hull_limit_maps():
    """{name: (label map, {label: hand-derived integers})}.
    wide   2 x 16384: label 1 the run of row 0 from column 100 to the last (a vertex at x = 16384), label 2 three pixels of row 1
           (first, middle and last column: the hull is the full 16384 x 1 rectangle).
    tall   16384 x 3: label 1 column 0 over the full height (a vertex at y = 16384; 16 385 levels), label 2 column 2 with a
           bulge into column 1 in the middle third (no rectangle: the host path alone)."""
    wide = np.zeros((2, 16384), np.int32)
    wide[0, 100:] = 1
    wide[1, [0, 8000, 16383]] = 2
    tall = np.zeros((16384, 3), np.int32)
    tall[:, 0] = 1
    tall[:, 2] = 2
    tall[5000:11000, 1] = 2
    for v in (wide, tall):
        v.setflags(write=False)
    return {"wide": (wide, {1: rect_integers(16284, 1), 2: rect_integers(16384, 1)}), "tall": (tall, {1: rect_integers(16384, 1)})}


def chunk_chain_points(cand, sign):
    """The points hull_chain_kernel's second pass merges for one side of one label: the levels are cut into 64 chunks and each
    chunk keeps its own chain.  cand: the candidate per corner level, None where the level has none."""
    levels = len(cand)
    c = (levels + 63) // 64
    kept = 0
    for lo in range(0, levels, c):
        ts = [t for t in range(lo, min(lo + c, levels)) if cand[t] is not None]
        kept += len(dh._chain(ts, [cand[t] for t in ts], sign))
    return c, kept


@functools.lru_cache(maxsize=None)
def hull_tall_parabolas():
    """16384 x 300, one label over the full height: in every chunk of 257 levels the leftmost pixels of the first 33 rows follow a
    parabola and the other rows are empty, so every one of those levels is a vertex of its chunk's left chain: more than 2048
    points for the second pass, which then runs in memory, at 16 385 levels.  The right side is one straight column."""
    h, w = 16384, 300
    lab = np.zeros((h, w), np.int32)
    r = np.arange(h)
    r = r[r % 257 < 33]
    lab[r, (r % 257 - 16) ** 2] = 1
    lab[r, w - 1] = 1
    lab[h - 1, 0] = lab[h - 1, w - 1] = 1
    lab.setflags(write=False)
    return lab


def left_candidates(lab, k):
    """Per corner level of label k (first row .. last row + 1): the leftmost pixel of the rows above and below, None without."""
    rows = np.flatnonzero((lab == k).any(axis=1))
    y0, y1 = int(rows[0]), int(rows[-1])
    xl = {int(y): int(np.flatnonzero(lab[y] == k)[0]) for y in rows}
    out = []
    for t in range(y0, y1 + 2):
        both = [xl[y] for y in (t - 1, t) if y in xl]
        out.append(min(both) if both else None)
    return out


# ---- Ripley --------------------------------------------------------------------------------------------------------------------

RIPLEY_SHAPE = (300, 401)
RIPLEY_TILE_COUNTS = (2049, 4100)   # one point in the second tile; two tiles and four points


def ripley_holes_window(h, w):
    """A window with a rectangular hole, two columns of holes across the 64-pixel seam and a corner pixel outside."""
    win = np.ones((h, w), np.uint8)
    win[h // 3:h // 3 + 5, w // 4:w // 4 + 9] = 0
    win[0, w - 1] = 0
    win[:, 64:66] = np.where(np.arange(h)[:, None] % 3 == 0, 0, 1)
    return win


@functools.lru_cache(maxsize=None)
def ripley_tile_points(N, windowed):
    """N points drawn inside the window (or the image), with coincident points inside a tile, across the first tile boundary and
    in the last tile -> (py, px, window)."""
    h, w = RIPLEY_SHAPE
    win = ripley_holes_window(h, w) if windowed else None
    py, px = (np.array(v) for v in ss.simulated_points(400 + N, 0, N, h, w, win))
    for a, b in coincident_pairs(N):                         # point a moves onto point b
        py[a], px[a] = py[b], px[b]
    return py, px, win


def coincident_pairs(N):
    """(a, b): inside the first tile; an i of the second tile on a j of the first; past two tiles also an i of the last tile
    on the last j of the first, and two neighbours in the last tile."""
    T = fx.RIPLEY_TILE
    return [(5, 4), (T, 3)] + ([(N - 1, T - 1), (N - 2, N - 3)] if N > 2 * T + 3 else [])


def assert_ripley_tiles_premise(N, py, px):
    T = fx.RIPLEY_TILE
    assert len(py) == N > T                                  # a second tile: t0 += RIPLEY_TILE runs
    assert N % T != 0                                        # ... and the last tile is a partial one
    if N > 2 * T:
        assert N % T == 4                                    # a third tile of one wave's worth of i
    pairs = coincident_pairs(N)
    assert any(a >= T > b for a, b in pairs) and (N < 2 * T or any(a >= 2 * T for a, b in pairs))
    assert all((py[a], px[a]) == (py[b], px[b]) for a, b in pairs)                       # t0 + j != i decides, not the distance


def pair_grid(max_points, S):
    """The workgroups per point set of spatial_pairs_kernel: grid_for(max_points, 4, max(1, 4096 / sets))."""
    return min(max(-(-max_points // 4), 1), max(1, fx.RIPLEY_PAIR_GROUPS // (1 + S)))


def assert_second_i_trip(N, S, max_points=None):
    """-> (workgroups, trips): more i than one trip of the grid handles."""
    groups = pair_grid(N if max_points is None else max_points, S)
    trips = -(-N // (4 * groups))
    assert -(-N // 4) > fx.RIPLEY_PAIR_GROUPS // (1 + S) and trips >= 2
    return groups, trips


RIPLEY_CAPACITY = 16384            # the droplet table's capacity in the flow: max_points of every Ripley call there
RIPLEY_SETS_CASE = dict(S=999, N=1049, R=8, h=96, w=130, seed=31)
RIPLEY_SETS_CHECKED = (0, 1, 996, 997, 998)                 # simulations whose rows are compared (and the observed pattern)


def assert_ripley_sets_premise(S, N):
    """(1 + S) N points pass one trip of spatial_sets_kernel; the points across index 1 048 576 belong to the last simulation."""
    P = fx.RIPLEY_SET_POINTS_PER_TRIP
    assert S == ss.MAX_SIMS and (1 + S) * N > P
    assert S * N < P - 64 and P + 64 < (1 + S) * N           # set S (simulation S - 1) holds the boundary, well inside
    assert S - 1 in RIPLEY_SETS_CHECKED


def ripley_limit_points(h, w):
    """The four corners, the middle of both long sides, and four points within reach of the far corners -> (py, px)."""
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    if h > w:
        pts += [(h // 2, 0), (h // 2, w - 1), (h - 4, 0), (h - 9, w - 1), (h - 9, 0), (h - 14, w - 1)]
    else:
        pts += [(0, w // 2), (h - 1, w // 2), (0, w - 4), (h - 1, w - 9), (0, w - 9), (h - 1, w - 14)]
    return [p[0] for p in pts], [p[1] for p in pts]


@functools.lru_cache(maxsize=None)
def long_table(k, h=96, w=130):
    """A droplet table of k droplets and a window that drops some of every 256 -> (area, sy, sx, window).  (random_case puts
    its last droplet outside the window; the table ends one before it, so its last entry may be kept.)"""
    from tests.spatial_ref import random_case
    area, sy, sx, window = random_case(h, w, k + 1, "noisy", seed=900 + k)
    return area[:k], sy[:k], sx[:k], window


def assert_table_chunks_premise(area, sy, sx, h, w, window, cap):
    """More than one chunk of 256; every chunk keeps a droplet, which the carried `kept` places in the output, and every chunk
    of more than one droplet drops one, so that the carried count is not the chunk's first index."""
    n = min(len(area), cap)
    assert n > fx.RIPLEY_TABLE_CHUNK
    a = np.maximum(area[:n], 1)
    y, x = (2 * sy[:n] + a) // (2 * a), (2 * sx[:n] + a) // (2 * a)
    keep = (y < h) & (x < w) & (window[np.minimum(y, h - 1), np.minimum(x, w - 1)] != 0)
    for lo in range(0, n, fx.RIPLEY_TABLE_CHUNK):
        part = keep[lo:lo + fx.RIPLEY_TABLE_CHUNK]
        assert part.any() and (len(part) == 1 or not part.all()), lo


# ---- border --------------------------------------------------------------------------------------------------------------------

BORDER_SHAPE = (1100, 960)
BORDER_RADIUS = 8


@functools.lru_cache(maxsize=None)
def border_masks(shape=BORDER_SHAPE):
    """Two different noise masks [2, h, w] float32, each with a plus-shaped component whose horizontal bar lies across raster
    index 1 048 576 (the first pixel of the second trip of the per-pixel kernels)."""
    from tests.border_ref import noise_mask
    h, w = shape
    masks = np.stack([noise_mask(h, w, 0.08, 41), noise_mask(h, w, 0.2, 42)])
    y, x = divmod(fx.BORDER_PIXELS_PER_TRIP, w)
    if 2 <= y < h - 2 and 8 <= x < w - 8:
        masks[:, y - 2:y + 3, x - 8:x + 9] = 0
        masks[0, y, x - 6:x + 7] = masks[0, y - 2:y + 3, x] = 1
        masks[1, y, x - 3:x + 2] = masks[1, y - 2:y + 3, x - 1] = 1
    masks.setflags(write=False)
    return masks


def assert_border_premise(masks):
    from scipy import ndimage
    n, h, w = masks.shape
    P = fx.BORDER_PIXELS_PER_TRIP
    assert n >= 2 and h * w > P                              # a second trip, and an image whose base is not 0
    assert not np.array_equal(masks[0], masks[1])
    for m in masks:
        flat = ndimage.label(m > 0.5)[0].ravel()
        assert flat[P - 1] > 0 and flat[P - 1] == flat[P]    # one run on both sides of the trip boundary
        part = np.flatnonzero(flat == flat[P])
        assert part[0] < P - w and part[-1] >= P + w         # ... of a component with rows above and below
    return h * w


# ---- outlines ------------------------------------------------------------------------------------------------------------------

def outline_rounds(max_len):
    """The leader and the rank rounds of launch_label_outlines: the smallest r, at most 31, with 2^r >= max_len."""
    r = 0
    while r < 31 and (1 << r) < max_len:
        r += 1
    return r


def crack_census(lab, n=None):
    """(ids, label) of every crack in ascending id, as the first lines of utils.droplet_outlines.outlines_numpy find them: the
    position of a crack in this list is the index ol_base_kernel gives it, and ids >> 2 is the corner it leaves."""
    lab = np.asarray(lab)
    h, w = lab.shape
    n = int(lab.max(initial=0)) if n is None else int(n)
    pad = np.zeros((h + 2, w + 2), np.int32)
    pad[1:-1, 1:-1] = np.where((lab >= 1) & (lab <= n), lab, 0)
    nw, ne, sw, se = pad[:-1, :-1], pad[:-1, 1:], pad[1:, :-1], pad[1:, 1:]
    own, left = np.stack((se, sw, nw, ne), axis=-1).ravel(), np.stack((ne, se, sw, nw), axis=-1).ravel()
    ids = np.flatnonzero((own > 0) & (own != left))
    return ids, own[ids]


def tiles(n, per=fx.OUTLINE_TILE):
    return -(-int(n) // per)


@functools.lru_cache(maxsize=None)
def outline_long_serpentine(shape=(1100, 960)):
    """One label, the rule of tests/test_gpu_outlines.py:serpentine: every other row full, joined alternately at the right and the
    left end.  One contour of 2 A + 2 cracks."""
    h, w = shape
    lab = np.zeros((h, w), np.int32)
    lab[0::2] = 1
    lab[1::4, w - 1] = 1
    lab[3::4, 0] = 1
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def outline_checkerboard(side=728):
    """Every other pixel a contour of its own (4 cracks, 4 vertices), in bands of 100 rows labelled 1, 2, 3, 1, ..."""
    r, c = np.mgrid[:side, :side]
    lab = (((r + c) % 2 == 0) * (1 + (r // 100) % 3)).astype(np.int32)
    lab.setflags(write=False)
    return lab


OUTLINE_BAR = (2 * 16384 + 2, 1, 0, 4, 2 * 16384, 2 * 16384)       # (E, no, nh, nv, F2, S2) of a 16384 x 1 bar


@functools.lru_cache(maxsize=None)
def outline_limit_maps():
    """{name: (label map, {label: hand-derived (E, no, nh, nv, F2, S2)})}, sides of 16384.
    tall   16384 x 2: label 1 column 0 over the full height (a vertex at y = 16384), label 2 in column 1 at the far end.
    wide   2 x 16384: label 1 row 0 over the full width (a vertex at x = 16384), label 2 in row 1 at the far end.
    Beside the bar one line of pixels is left, where neither a one-pixel hole nor a notch fits: label 2 is two pixels, a gap, and
    the last pixel: two contours that touch the bar and the last corner (16384, 2) or (2, 16384).  The bar: 2 A + 2 cracks, one
    outer contour, four vertices, twice its area."""
    tall = np.zeros((16384, 2), np.int32)
    tall[:, 0] = 1
    tall[[16380, 16381, 16383], 1] = 2
    wide = np.ascontiguousarray(tall.T)
    for v in (tall, wide):
        v.setflags(write=False)
    two = (6 + 4, 2, 0, 8, 4 + 2, 4 + 2)                     # a 2 x 1 piece and a pixel
    return {"tall": (tall, {1: OUTLINE_BAR, 2: two}), "wide": (wide, {1: OUTLINE_BAR, 2: two})}


OUTLINE_BLOB_SHAPE, OUTLINE_BLOB_SEED = (1040, 1388), 3


@functools.lru_cache(maxsize=None)
def outline_blob_labels():
    """A label map of the flow's full image size: the components of a blob mask, numbered as cap_labels numbers its own."""
    lab = fx.components(fx.blob_mask(*OUTLINE_BLOB_SHAPE, seed=OUTLINE_BLOB_SEED))
    lab.setflags(write=False)
    return lab


OUTLINE_MAPS = {"serpentine": outline_long_serpentine, "checkerboard": outline_checkerboard,
                "tall": lambda: outline_limit_maps()["tall"][0], "wide": lambda: outline_limit_maps()["wide"][0],
                "blobs": outline_blob_labels, **{f"{h}x{w}": (lambda s=(h, w): fx.cap_labels(s)[0]) for h, w in fx.CAP_SHAPES}}


@functools.lru_cache(maxsize=None)
def outline_ref(name):
    """(label map, the follower's record for its labels 1..max) of OUTLINE_MAPS[name]: computed once, shared, read-only."""
    from utils.droplet_outlines import outlines_numpy
    lab = OUTLINE_MAPS[name]()
    ref = outlines_numpy(lab, int(lab.max()))
    for v in (*ref["rows"].values(), *ref["contours"].values(), ref["x"], ref["y"]):
        v.setflags(write=False)
    return lab, ref


def outline_counts(lab, ref):
    """(corners, cracks, contours, vertices, longest contour) of a map and its follower's record."""
    h, w = lab.shape
    c = ref["contours"]
    return (h + 1) * (w + 1), int(c["length"].sum()), len(c["label"]), len(ref["x"]), int(c["length"].max(initial=0))


def assert_outline_serpentine_premise(lab, ref):
    """One contour longer than one trip of the crack-side loops, so that pointer jumping crosses the trip boundary; more corner
    tiles than one trip of the crack scan; a round count the small fixtures do not reach."""
    corners, cracks, contours, vertices, longest = outline_counts(lab, ref)
    A = int(lab.sum())
    assert set(np.unique(lab).tolist()) == {0, 1} and contours == 1 and longest == cracks == 2 * A + 2
    assert cracks == len(crack_census(lab)[0]) > fx.OUTLINE_CRACKS_PER_TRIP
    assert tiles(corners) > fx.OUTLINE_SCAN_TILES_PER_TRIP and corners <= fx.OUTLINE_CORNERS_PER_TRIP
    assert outline_rounds(longest) > 15 and outline_rounds(fx.OUTLINE_CRACKS_PER_TRIP) == outline_rounds(longest) - 1
    return corners, tiles(corners), cracks, contours, vertices, outline_rounds(longest)


def assert_outline_checkerboard_premise(lab, ref):
    """More cracks, contours and crack tiles than one trip holds while the corners stay within one trip of every corner-side
    loop; contours that start on the second trip; more than one label on the first, and a band that holds the boundary."""
    corners, cracks, contours, vertices, longest = outline_counts(lab, ref)
    P = fx.OUTLINE_CRACKS_PER_TRIP
    assert tiles(corners) <= fx.OUTLINE_SCAN_TILES_PER_TRIP and corners <= fx.OUTLINE_CORNERS_PER_TRIP
    assert cracks > P and tiles(cracks) > fx.OUTLINE_SCAN_TILES_PER_TRIP and vertices > P and contours > P // 4
    ids, own = crack_census(lab)
    assert len(ids) == cracks
    h, w = lab.shape
    c = ref["contours"]
    start = (ref["y"][c["first"]].astype(np.int64) * (w + 1) + ref["x"][c["first"]]) * 4         # the E crack of the start's tail
    index = np.searchsorted(ids, start)
    assert np.array_equal(ids[index], start) and (np.diff(index) > 0).all()
    late = index >= P
    assert late.any() and not late.all() and index[late].min() - P < 4                           # a contour across the boundary, or next to it
    assert len(np.unique(own[:P])) > 1                       # a label band changes before the boundary ...
    assert own[P - 1] == own[P] and (own[:P] == own[P]).sum() > w                                # ... and the one across it began well before
    return corners, cracks, contours, vertices, tiles(cracks), int(late.sum())


def assert_outline_corner_grid_premise(lab, ref):
    """More corners than one trip of ol_successor_kernel, three trips of the crack scan, and a label with cracks that leave
    corners on both sides of corner 2 097 152: from the crack census, not from the pixels.  -> (corners, corner tiles, labels,
    cracks, contours, holes, labels with a crack past the boundary, those of them with a crack before it)."""
    corners, cracks, contours, vertices, longest = outline_counts(lab, ref)
    P = fx.OUTLINE_CORNERS_PER_TRIP
    assert corners > P and tiles(corners) > 2 * fx.OUTLINE_SCAN_TILES_PER_TRIP
    ids, own = crack_census(lab)
    assert len(ids) == cracks <= fx.OUTLINE_CRACKS_PER_TRIP
    past = np.unique(own[(ids >> 2) >= P])
    both = np.intersect1d(past, np.unique(own[(ids >> 2) < P]))
    assert len(both) >= 1
    return corners, tiles(corners), int(lab.max()), cracks, contours, int((ref["contours"]["S2"] < 0).sum()), len(past), len(both)


def assert_outline_limit_premise(name, lab, ref, hand):
    """A side of 16384 with a vertex on its last lattice line, and label 2 at the far corner."""
    h, w = lab.shape
    assert (h, w) == ((16384, 2) if name == "tall" else (2, 16384)) and int(lab.max()) == 2
    far = ref["y"] if name == "tall" else ref["x"]
    c = ref["contours"]
    owner = np.repeat(c["label"], c["nv"])
    assert far[owner == 1].max() == 16384 and far[owner == 2].max() == 16384 and far[owner == 1].min() == 0
    assert (ref["x"].max(), ref["y"].max()) == (w, h)
    for k, ints in hand.items():
        assert tuple(int(ref["rows"][q][k - 1]) for q in ("E", "no", "nh", "nv", "F2", "S2")) == ints, (name, k)
