"""GPU: the grid-stride loops of the droplet stages on their second trip.  A launcher caps its grid; past the cap a thread
(or a wave) comes round again with `index += stride`.  Per capped kernel: the cap, and the test whose shape exceeds it.

  label_props_kernel (shape.hip)        8192 blocks x 4 waves = 32 768 units of 64 pixels of a row.  8200 x 257 (5 units per row,
                                        the last of one pixel: 41 000 units) and 600 x 3521 (56 per row, the last of one pixel:
                                        33 600 units): test_label_props_past_the_grid_cap.
  match_overlap_kernel (match.hip)      the same cap and shapes: test_label_overlap_past_the_grid_cap.
  label_props_init_kernel (shape.hip)   1024 blocks x 256 threads = 262 144 words, max_out > 18 724: max_out = 20 000 in
                                        test_label_props_initialises_twenty_thousand_numbers (production passes 65 536).
  the kernels of csrc/pair_table.h, compiled once into match.hip (PairAdd) and once into neighbors.hip (PairMin).  Every sort
  kernel sizes its network by pair_sort_size(): the power of two that holds the ENTRIES, at most the capacity's.  So a cap of
  the sort is passed only by the number of entries, never by the capacity; a roomy capacity buys launches that return at once.
    pair_init_kernel                    2048 blocks x 256 = 524 288 hash slots (a power of two >= 2 max_pairs) and sort keys:
                                        passed by capacity alone.  Every max_pairs = h * w call at full size, and
                                        test_label_overlap_with_room_for_every_pixel (8 388 608 slots); in neighbors.hip
                                        test_neighbors_past_the_label_and_pair_grids (max_pairs = 2^21: 4 194 304 slots).
    pair_compact_kernel                 the same grid over the slots, and the same tests; its ENTRIES pass 524 288 only in the
                                        two tests just named (2 107 400 / 2 112 600 and 1 123 500 entries).
    pair_sort_local_kernel              one block per chunk of 4096 entries, no loop over the grid.  A block other than block 0
                                        and the merge-tail form (k_lo = k_hi > 4096) need more than 4096 entries:
                                        tests/test_gpu_match.py::test_list_lengths_around_the_sort_chunks and
                                        tests/test_gpu_neighbors.py::test_lattices_of_more_pairs_than_a_sort_chunk.
    pair_sort_global_kernel             runs at all only past 4096 entries (the two tests just named).  4096 blocks x 256 =
                                        1 048 576 compare-exchanges, half the network: a second trip needs more than 2^21
                                        ENTRIES.  unique_pair_labels at 8200 x 257 and 600 x 3521 makes every pixel a pair:
                                        h * w > 2^21 entries, a network of 2^22: test_label_overlap_with_room_for_every_pixel.
                                        (Its blob maps, and tests/test_gpu_match.py::test_full_size_with_room_for_every_pixel,
                                        ask for that capacity with 200-999 and 1955 entries: n <= 2048, no global pass.)
                                        The neighbors.hip copy stays on its first trip: 1 123 500 entries, a network of 2^21.
    pair_emit_kernel                    2048 x 256 = 524 288 entries: the same two tests, one per copy.
  neighbors_pairs_kernel (neighbors.hip)   2048 x 256 = 524 288 sorted pairs: lattice_map(1500, 1500, 2) at G = 2 has 1 123 500,
                                        united into ONE cluster: test_neighbors_past_the_label_and_pair_grids.
  neighbors_init_kernel, neighbors_flatten_kernel, neighbors_size_kernel   2048 x 256 = 524 288 labels: the same map has
                                        562 500: the same test.
  neighbors_scan_kernel                 4096 blocks x 4 waves = 16 384 border pixels a trip: already passed by
                                        tests/test_gpu_neighbors.py::test_more_border_pixels_than_the_scan_grid (60 000), and by
                                        the 562 500 border pixels here.
  neighbors_border_kernel               8192 blocks x 4 waves = 32 768 tiles of 16 x 64 pixels = 33 554 432 pixels a trip.  A
                                        second trip needs more than 33.5 M pixels (5793 x 5793): a 134 MB label map and as
                                        much again for the border list.  Deliberately not reached; 1500 x 1500 is 2256 tiles.
  the per-pixel loops of split.hip, clean.hip, ccl.hip, density.hip   4096 blocks x 256 = 1 048 576 pixels: exceeded by every
                                        1040 x 1388 test of tests/test_gpu_split.py, test_gpu_clean.py, test_gpu_shape.py and
                                        test_gpu_density.py.

The label maps (tests/droplet_edge_fixtures.py:cap_labels) are the components of a blob mask: a few hundred droplets that
cross the 64-pixel seams, some of them the row where the second trip starts, and one in the last rows and columns.  Host
references at these shapes, timed on the CPU: label_props_numpy 0.25 s, overlap_table_numpy 0.03 s (0.2 s on
unique_pair_labels), the plain loops of tests/match_ref.py 0.5 s, offset_pairs and neighbor_columns on the 1500 x 1500 lattice
1.3 s -- the shapes the cap asks for are kept."""
import numpy as np
import pytest

from tests import droplet_edge_fixtures as fx
from tests import neighbors_ref
from tests.match_ref import overlap_table_ref
from tests.test_gpu_match import assert_arrays_equal_host_path, device_overlap, host_table
from tests.test_gpu_neighbors import device_neighbors_arrays
from tests.test_gpu_shape import NQ, assert_props_equal
from tests.test_match_cpu import kmax
from tests.test_shape_cpu import gray_plane
from utils import droplet_neighbors as dn
from utils import droplet_shape as sh

pytestmark = pytest.mark.gpu

IDS = [f"{h}x{w}" for h, w in fx.CAP_SHAPES]
_plain = {}


def plain_table(shape):
    """The contingency table by the plain loops of tests/match_ref.py, once per shape."""
    if shape not in _plain:
        A, B = fx.cap_labels(shape)
        _plain[shape] = overlap_table_ref(A.tolist(), B.tolist(), kmax(A), kmax(B))
    return _plain[shape]


def assert_reaches_the_second_trip(lab):
    h, w = lab.shape
    assert h * ((w + 63) // 64) > fx.WAVE_UNITS_PER_TRIP and w % 64 == 1
    late = fx.labels_past_unit(lab)
    assert len(late) >= 1                                                  # a labelled run in a unit >= 32 768
    assert len(np.intersect1d(late, fx.labels_before_unit(lab))) >= 1      # a droplet on both sides of the trip boundary
    assert ((lab[:, 63] == lab[:, 64]) & (lab[:, 63] > 0)).any()           # ... and across a 64-pixel seam
    assert lab[h - 1, w - 1] > 0                                           # the last unit holds one pixel, and it is labelled


@pytest.mark.parametrize("with_gray", [False, True], ids=["no_gray", "gray"])
@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_label_props_past_the_grid_cap(shape, with_gray):
    lab = fx.cap_labels(shape)[0]
    assert_reaches_the_second_trip(lab)
    assert_props_equal(lab, gray_plane(*shape, seed=5) if with_gray else None)


def test_label_props_initialises_twenty_thousand_numbers():
    """max_out = 20 000: 280 000 words, the init kernel's second trip.  Every row past the last label holds its initial value."""
    lab = fx.few_dozen_labels()
    k = kmax(lab)
    assert 24 <= k <= 100 and NQ * 20000 > 1024 * 256
    for gray in (None, gray_plane(*lab.shape)):
        got = assert_props_equal(lab, gray, max_out=20000)
        assert np.array_equal(got[:, k:], fx.initial_rows(NQ, 20000 - k, sh.QUANTITIES, sh.MIN_INIT, sh.MAX_INIT))


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_label_overlap_past_the_grid_cap(shape):
    """A capacity of a few thousand pairs: the overlap kernel alone is past its cap."""
    A, B = fx.cap_labels(shape)
    assert_reaches_the_second_trip(A)
    assert_reaches_the_second_trip(B)
    ka, kb = kmax(A), kmax(B)
    ref = host_table(A, ka, B, kb)
    assert ref == plain_table(shape) and 200 <= len(ref) <= 999
    assert device_overlap(A, ka, B, kb, max_pairs=4 * (ka + kb) + 64) == (len(ref), ref)


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_label_overlap_with_room_for_every_pixel(shape):
    """max_pairs = h * w > 2^21: 2^23 hash slots (init and compact on their second trip).  On the blob maps the list is a few
    hundred entries and the sort a short one; on unique_pair_labels every pixel is an entry: a network of 2^22, so every global
    compare-exchange pass takes a second trip over its 2^21 pairs, and compact and emit pass their caps by entries."""
    A, B = fx.cap_labels(shape)
    h, w = shape
    assert 1 << 21 < h * w <= 1 << 22
    ka, kb = kmax(A), kmax(B)
    assert device_overlap(A, ka, B, kb) == (len(plain_table(shape)), plain_table(shape))
    ref, _ = assert_arrays_equal_host_path(*fx.unique_pair_labels(shape))
    assert len(ref[0]) == h * w > 1 << 21


def test_neighbors_past_the_label_and_pair_grids():
    """562 500 single-pixel droplets two pixels apart, 1 123 500 pairs at G = 2: the per-label kernels and neighbors_pairs_kernel
    past 2048 x 256, more than a million pairs united into one cluster, every nearest contact a tie the smaller label wins."""
    h, w, step, G, k, n = neighbors_ref.CAP_LATTICE
    lab, _ = neighbors_ref.lattice_map(h, w, step)
    pairs = neighbors_ref.offset_pairs(lab, k, G)
    cols = dn.neighbor_columns(pairs, k)
    assert k > fx.PAIR_GRID_PER_TRIP and len(pairs[0]) == n > 2 * fx.PAIR_GRID_PER_TRIP
    count, got, gcols, _ = device_neighbors_arrays(lab, k, G, max_pairs=1 << 21)
    assert count == n
    for x, y in zip(got, pairs):
        assert np.array_equal(x, y), np.flatnonzero(x != y)[:5]
    for q in dn.COLUMN_NAMES:
        assert np.array_equal(gcols[q], cols[q]), (q, np.flatnonzero(gcols[q] != cols[q])[:5])
    assert (gcols["cluster"] == 1).all() and (gcols["cluster_size"] == k).all() and (gcols["nn_d2"] == 4).all()
    assert gcols["degree"].min() == 2 and gcols["degree"].max() == 4 and (gcols["nn_label"] >= 1).all()
