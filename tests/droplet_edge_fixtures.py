"""Inputs of tests/test_gpu_grid_caps.py, of the long-list tests of tests/test_gpu_match.py (pair_count_labels,
unique_pair_labels) and of the C-ABI density tests (tests/test_gpu_density.py), and the host-side rules
they are checked with; tests/test_droplet_edges_cpu.py pins what each of them is for."""
import functools

import numpy as np
from scipy import ndimage

from utils import density as hd

WAVE_UNITS_PER_TRIP = 8192 * 4    # label_props_kernel / match_overlap_kernel: 8192 blocks of 4 waves, one 64-pixel unit per wave
CAP_SHAPES = ((8200, 257), (600, 3521))
# Mirrors of the caps of hull.hip, spatial.hip and border.hip; tests/test_droplet_edges_cpu.py reads the constexpr values and the
# launch lines from the sources and checks every one of them.  The fixtures that pass them are in tests/cap_fixtures.py.
HULL_MAX_GROUPS = 4096            # hull_caliper_kernel: workgroups of 4 waves, one label per wave
HULL_MAX_CHAINS = 1 << 15         # hull_chain_kernel: one-wave workgroups, one per (label, side)
HULL_LDS_POINTS = 2048            # levels, and chunk vertices, of one side that a chain pass holds in LDS
HULL_LABELS_PER_TRIP = min(HULL_MAX_CHAINS // 2, HULL_MAX_GROUPS * 4)     # label k and label k + 16 384 share a wave
HULL_WORDS_PER_TRIP = 1024 * 256  # hull_init_kernel (words of the output) and hull_fill_kernel (used slots)
RIPLEY_TILE = 2048                # spatial_pairs_kernel: packed points per LDS tile
RIPLEY_PAIR_GROUPS = 4096         # ... its grid: max(1, 4096 // (1 + S)) workgroups of 4 waves per point set, one i per wave
RIPLEY_SET_POINTS_PER_TRIP = 4096 * 256    # spatial_sets_kernel: one thread per point of every set
RIPLEY_TABLE_CHUNK = 256          # spatial_points_kernel: droplets per step of its one workgroup
BORDER_PIXELS_PER_TRIP = 4096 * 256        # border_init / border_merge / border_flatten, per image
# ... and of outlines.hip
OUTLINE_TILE = 1024               # OL_THREADS * OL_ITEMS: corners of a census tile, cracks of a contour tile
OUTLINE_SCAN_TILES_PER_TRIP = 1024         # scan_plane (wave_ops.h): one workgroup of 1024, one tile count per thread and trip
OUTLINE_CRACKS_PER_TRIP = 4096 * 256       # ol_leader / ol_cut / ol_rank / ol_vertices: OL_MAX_GRID blocks of 256 threads
OUTLINE_CORNERS_PER_TRIP = 8192 * 256      # ol_successor_kernel
OUTLINE_INIT_WORDS_PER_TRIP = 1024 * 256   # ol_init_kernel: words of the 6 output rows


def unit_of(y, x, w):
    """The wave unit that handles pixel (y, x) of an image w wide: 64 consecutive pixels of one row, numbered row by row."""
    return y * ((w + 63) // 64) + x // 64


def labels_past_unit(lab, first_unit=WAVE_UNITS_PER_TRIP):
    """The labels (> 0) that have a pixel in a unit >= first_unit: the units a capped grid reaches on a later trip only."""
    h, w = lab.shape
    yy, xx = np.nonzero(lab > 0)
    late = unit_of(yy, xx, w) >= first_unit
    return np.unique(lab[yy[late], xx[late]])


def labels_before_unit(lab, first_unit=WAVE_UNITS_PER_TRIP):
    h, w = lab.shape
    yy, xx = np.nonzero(lab > 0)
    early = unit_of(yy, xx, w) < first_unit
    return np.unique(lab[yy[early], xx[early]])


def blob_mask(h, w, seed, sigma=12.0, frac=0.2):
    """Thresholded smoothed noise (as tests/test_split_cpu.py:noise_mask, coarser: a few hundred blobs on two megapixels),
    with a 3 x 3 droplet in the last rows and columns."""
    f = ndimage.gaussian_filter(np.random.default_rng(seed).random((h, w)), sigma)
    m = (f > np.quantile(f, 1.0 - frac)).astype(np.uint8)
    m[h - 5:, w - 5:] = 0
    m[h - 3:, w - 3:] = 1
    return m


def components(mask):
    """The 4-connected components of a mask as an int32 label map, numbered in raster order."""
    return ndimage.label(mask, ndimage.generate_binary_structure(2, 1))[0].astype(np.int32)


@functools.lru_cache(maxsize=None)
def cap_labels(shape):
    """-> (A, B): the 4-connected components of a blob mask of `shape` and of the same mask moved down 2 and right 1, both
    with the corner droplet, numbered in raster order."""
    h, w = shape
    m = blob_mask(h, w, seed=h)
    moved = np.zeros_like(m)
    moved[2:, 1:] = m[:h - 2, :w - 1]
    moved[h - 3:, w - 3:] = 1
    return components(m), components(moved)


PAIR_SORT_CHUNK = 4096            # pair_table.h: the entries one workgroup sorts in LDS; a longer list takes the global passes
PAIR_GRID_PER_TRIP = 2048 * 256   # pair_init / pair_compact / pair_emit, neighbors_pairs and the per-label kernels of neighbors.hip
PAIR_SHAPE = (96, 256)
PAIR_B_LABELS = 61                # labels of the second map of pair_count_labels
PAIR_B_PER_A = 5                  # partners of one label of the first map


def pair_count_pairs(E):
    """The construction of pair_count_labels -> int64 (a, b, pixels) of pair p = 0..E-1, in (a, b) order.  Label a = p // 5 + 1
    has the five partners b = ((p % 5) * 12 + 7 (a - 1)) % 61 + 1, distinct because 12 j < 61 for j < 5; a label b meets many a.
    Every third pair has a second pixel, every eleventh one more."""
    p = np.arange(int(E), dtype=np.int64)
    a = p // PAIR_B_PER_A + 1
    b = ((p % PAIR_B_PER_A) * 12 + 7 * (a - 1)) % PAIR_B_LABELS + 1
    n = 1 + (p % 3 == 0) + (p % 11 == 0)
    order = np.lexsort((b, a))
    return a[order], b[order], n[order].astype(np.int64)


@functools.lru_cache(maxsize=None)
def pair_count_labels(E, shape=PAIR_SHAPE):
    """-> (A, B): int32 label maps of `shape` with exactly E distinct overlapping (a, b) pairs, those of pair_count_pairs(E), at
    pixel positions shuffled with a fixed seed (the pixels of one pair lie apart: the combine step of the insert runs, not
    only the run length).  Of the pixels left over a third carries a label on the first map only, a third on the second only."""
    h, w = shape
    a, b, n = pair_count_pairs(E)
    total = int(n.sum())
    assert total <= h * w
    pos = np.random.default_rng(1000 + int(E)).permutation(h * w)
    A, B = np.zeros(h * w, np.int32), np.zeros(h * w, np.int32)
    A[pos[:total]] = np.repeat(a, n)
    B[pos[:total]] = np.repeat(b, n)
    rest = pos[total:]
    A[rest[0::3]] = 1 + rest[0::3] % int(a.max())              # a label over background of the other map: no pair
    B[rest[1::3]] = 1 + rest[1::3] % PAIR_B_LABELS
    A, B = A.reshape(h, w), B.reshape(h, w)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def unique_pair_labels(shape):
    """-> (A, B): A a seeded permutation of 1..h*w, B = (i % 5) + 1 at linear index i.  Every pixel is a pair of its own: the
    list is h * w long."""
    h, w = shape
    A = (1 + np.random.default_rng(h + w).permutation(h * w)).astype(np.int32).reshape(h, w)
    B = (np.arange(h * w) % 5 + 1).astype(np.int32).reshape(h, w)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


RUN_EDGE_MAX_OUT = 13             # the labels of run_edge_labels that count; RUN_EDGE_SKIPPED lies above it
RUN_EDGE_SKIPPED = 20


def run_edge_labels():
    """A 6 x 130 map (two full 64-lane chunks and a chunk with 2 live lanes) for the run helpers of csrc/wave_ops.h, which every
    per-row stage shares.  Row 0: one label over the whole row (runs of 64, 64 and 2: a run mask of all 64 lanes).  Row 1: a new
    label at every pixel (64 heads in a wave).  Row 2: the label changes exactly at x = 63|64 and 127|128, and one label lives
    at x = 129 only.  Row 3: background but for x = 0, x = 63 and x = 64.  Row 4: a label above RUN_EDGE_MAX_OUT inside a run of
    a valid one, which it splits.  Row 5: background.  tests/test_droplet_edges_cpu.py checks each of these."""
    lab = np.zeros((6, 130), np.int32)
    lab[0] = 1
    lab[1] = 2 + np.arange(130) % 5                             # 2..6
    lab[2, :64], lab[2, 64:128], lab[2, 128], lab[2, 129] = 7, 8, 9, 10
    lab[3, 0], lab[3, 63:65] = 11, 12
    lab[4, 40:120] = 13
    lab[4, 70] = RUN_EDGE_SKIPPED
    lab.setflags(write=False)
    return lab


def moved_one_pixel(lab):
    """The map one pixel to the right (one pixel down where it is one column wide), zeros moving in: the second map of the
    overlap and boundary cases, whose runs end one lane after the first map's."""
    out = np.zeros_like(lab)
    if lab.shape[1] > 1:
        out[:, 1:] = lab[:, :-1]
    else:
        out[1:] = lab[:-1]
    return out


def few_dozen_labels():
    """A 96 x 130 map of split droplets (touching labels), a few dozen of them: the map of the large-max_out test."""
    from tests.test_shape_cpu import split_labels
    from tests.test_split_cpu import noise_mask
    return split_labels(noise_mask(96, 130, seed=96, sigma=2.0))


def initial_rows(nq, cap, quantities, min_init, max_init):
    """[nq][cap] int64 as unetdc_label_props leaves the rows of numbers without pixels: minima at min_init, maxima at max_init,
    sums and counts 0."""
    out = np.zeros((nq, cap), np.int64)
    for j, q in enumerate(quantities):
        out[j] = min_init if q.startswith("min_") else max_init if q.startswith("max_") else 0
    return out


def ring_counts_of_table(area, sumy, sumx, cap, roi, nb_layers):
    """The ring counts unetdc_density_maps must give for a droplet table of which it may read the first `cap` entries only:
    the host ring rule (utils.density.radial_map) on the truncated table."""
    cx, cy, _ = hd.roi_centroid(roi)
    a = np.asarray(area[:cap], dtype=np.float64)
    cen = (np.asarray(sumy[:cap], dtype=np.float64) / a, np.asarray(sumx[:cap], dtype=np.float64) / a)
    return hd.radial_map(np.zeros(roi.shape, np.uint8), roi, nb_layers, cy, cx, centroids=cen)[2]


BOUND_SHAPE = (121, 161)          # centre (60, 80), corners at sqrt(60^2 + 80^2) = 100: with L = 10 the ring bounds are 10 i
BOUND_LAYERS = 10
# (pixels of one droplet, its centroid distance, the ring it belongs to or -1)
BOUND_DROPLETS = (
    ([(0, 0)], 100.0, 9),                                   # the farthest ROI pixel: d = b_L, the last ring
    ([(12, 16)], 80.0, 7),                                  # (48, 64): d = b_8 -> ring 7, not 8
    ([(30, 120)], 50.0, 4),                                 # (30, 40): d = b_5 -> ring 4
    ([(60, 80)], 0.0, -1),                                  # the centroid itself: b_0 < d fails, no ring
    ([(60, 90)], 10.0, 0),                                  # d = b_1 -> ring 0
    ([(60, 99), (60, 100), (60, 101)], 20.0, 1),            # centroid from sums / area: d = b_2 -> ring 1
    ([(60, 111)], 31.0, 3),                                 # off a bound: (30, 40]
    ([(89, 80), (90, 80), (91, 80)], 30.0, 2),              # vertical, centroid from sums / area: d = b_3 -> ring 2
)


def bound_case():
    """A flat grey image: Otsu finds no split, the ROI is the whole image, its centroid the centre pixel and the largest ROI
    distance exactly 100.  -> (rgb, mask, per-droplet expected rings in label order, expected ring counts).
    The ROI is symmetric about the centre, maxd = 100 and maxd / L = 10 are integers, so every bound i * (maxd / L) is exact in
    fp64 and equals the distance of a droplet placed 10 i pixels from the centre along an axis or a 3-4-5 direction."""
    h, w = BOUND_SHAPE
    rgb = np.full((h, w, 3), 77, np.uint8)
    mask = np.zeros((h, w), np.uint8)
    drops = BOUND_DROPLETS
    for pix, _, _ in drops:
        for y, x in pix:
            mask[y, x] = 1
    order = sorted(range(len(drops)), key=lambda i: min(y * w + x for y, x in drops[i][0]))
    rings = [drops[i][2] for i in order]
    counts = np.bincount([r for r in rings if r >= 0], minlength=BOUND_LAYERS).astype(np.int64)
    return rgb, mask, rings, counts
