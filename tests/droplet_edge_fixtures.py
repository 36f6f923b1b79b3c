"""Inputs of tests/test_gpu_grid_caps.py and of the C-ABI density tests (tests/test_gpu_density.py), and the host-side rules
they are checked with; tests/test_droplet_edges_cpu.py pins what each of them is for."""
import functools

import numpy as np
from scipy import ndimage

from utils import density as hd

WAVE_UNITS_PER_TRIP = 8192 * 4    # label_props_kernel / match_overlap_kernel: 8192 blocks of 4 waves, one 64-pixel unit per wave
CAP_SHAPES = ((8200, 257), (600, 3521))


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


@functools.lru_cache(maxsize=None)
def cap_labels(shape):
    """-> (A, B): the 4-connected components of a blob mask of `shape` and of the same mask moved down 2 and right 1, both
    with the corner droplet, numbered in raster order."""
    h, w = shape
    m = blob_mask(h, w, seed=h)
    moved = np.zeros_like(m)
    moved[2:, 1:] = m[:h - 2, :w - 1]
    moved[h - 3:, w - 3:] = 1
    s = ndimage.generate_binary_structure(2, 1)
    return ndimage.label(m, s)[0].astype(np.int32), ndimage.label(moved, s)[0].astype(np.int32)


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
