"""Constructed inputs of the image-side edge tests (tests/test_gpu_augment.py, test_gpu_preprocess.py, test_gpu_droplets.py),
built on the host so that tests/test_image_edges_cpu.py can prove each one does what its GPU test relies on."""
import numpy as np

from tests import augment_ref as ref

GATHER_MAX_BATCH = 32             # csrc/kernels.h AUG_MAX_BATCH: records per gather launch
FIELDS_MAX_SEEDS = 64             # csrc/kernels.h AUG_MAX_SEEDS: field slots per row / column-pass launch
NEAR_TIE = 1e-3                   # |frac - 0.5| below this on either axis: the order-0 mask tap may fall either way
NEAR_TIE_CAP = 0.02               # ... an exemption, so at most this share of a sample's pixels may claim it


# ---- rolling ball: rounding ties in the normalise step ---------------------------------------------------------------------
TIE_EXPECTED = [26, 51, 76, 102, 128, 153, 178, 204, 230, 255]        # round-half-even of v * 25.5, v = 1 .. 10
TIE_HALF_UP = [26, 51, 77, 102, 128, 153, 179, 204, 230, 255]


def tie_image(channels):
    """Black [40, 60, channels] uint8 image with isolated single pixels of value 1 .. 10 (another order in every channel):
    any opening removes them, so corrected = image, min 0, max 10, scale 25.5 -- 3 and 7 land exactly on .5."""
    img = np.zeros((40, 60, channels), np.uint8)
    for c in range(channels):
        for j in range(10):
            img[4 + 8 * (j // 5) + 16 * (c % 2), 6 + 11 * (j % 5), c] = 1 + (j + 3 * c) % 10
    return img


def tie_positions(img, c):
    """{value: (y, x)} of the ten marked pixels of channel c."""
    ys, xs = np.nonzero(img[..., c])
    return {int(img[y, x, c]): (int(y), int(x)) for y, x in zip(ys, xs)}


# ---- augmentation: batches that cross the launch chunks ----------------------------------------------------------------------
def chunk_params(n, ncache, seed, elastic=()):
    """n draw_params-style records with flips, k, brightness / contrast and sources drawn independently per sample (nothing
    repeats with the chunk length); samples in `elastic` draw a field, each with its own seed.  -> (params, sources)."""
    r = np.random.default_rng(seed)
    ps = []
    for j in range(n):
        bc = bool(r.random() < 0.5)
        ps.append(dict(hflip=bool(r.random() < 0.5), vflip=bool(r.random() < 0.5), k=int(r.integers(0, 4)), bc=bc,
                       alpha=1.0 + r.uniform(-0.2, 0.2) if bc else 1.0, beta=r.uniform(-0.2, 0.2) if bc else 0.0,
                       elastic=j in elastic, field_seed=int(r.integers(0, 2 ** 32))))
    return ps, [int(v) for v in r.integers(0, ncache, n)]


def field_seeds(n):
    """n distinct 32-bit seeds, not a progression."""
    return [int(v) for v in ref.fmix32(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761))]


# name -> (samples, elastic sample indices, side, sigma, alpha): the elastic gather fixtures
ELASTIC_SIDE = 48
ELASTIC_CASES = {
    # 66 elastic of 70 samples: field slots cross the 32-record gather launch AND the 64-seed field launch
    "chunks": (70, tuple(j for j in range(70) if j not in (5, 33, 50, 64)), ELASTIC_SIDE, 3.0, 40.0),
    # |d| > 2 side for part of the field: the reflection wraps more than one period
    "long": (4, (0, 1, 2, 3), 24, 3.0, 2500.0),
}


def near_tie(dx, dy):
    """The pixels whose order-0 tap is within NEAR_TIE of a rounding tie on either axis (dx, dy: float64 displacements)."""
    h, w = dx.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    frac = lambda c: np.abs((c - np.floor(c)) - 0.5)                     # noqa: E731
    return (frac(yy + dy) < NEAR_TIE) | (frac(xx + dx) < NEAR_TIE)


# ---- connected components: areas on either side of min_area ----------------------------------------------------------------
def area_boundary_mask(min_area, h=23, w=27):
    """uint8 [h, w] mask (w not a multiple of 4) of separate 4-connected components with areas min_area - 1, min_area and
    min_area + 1, three of each: a bar that ends at the last column, a bar that starts at column 0 of the NEXT row (adjacent
    in linear index, not in the image) and a bent one whose first pixel lies above its far end."""
    m = np.zeros((h, w), np.uint8)
    y = 0
    for a in (min_area + 1, min_area - 1, min_area):
        m[y, w - a:] = 1
        m[y + 1, :a] = 1
        y += 3
    for a in (min_area, min_area + 1, min_area - 1):
        m[y, 5 + max(a - 2, 0)] = 1
        m[y + 1, 5:5 + a - 1] = 1
        y += 3
    return m
