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

  hull.hip.  Label k and label k + 16 384 share one wave of the chain and of the caliper kernel, and with it s_count, s_pts, s_lvl.
    hull_init_kernel                    1024 x 256 = 262 144 words over 5 max_out: max_out > 52 428.  max_out = 65 536 (what
                                        mask_and_droplets passes): test_hull_sparse_high_label_numbers, where 65 522 numbers without
                                        pixels keep the zeros, before and after a 0xFF prefill.
    hull_extent_kernel, hull_rows_kernel   8192 x 4 waves = 32 768 units, the frame of label_props_kernel: 41 000 and 33 600 units in
                                        test_label_hull_past_the_grid_cap.
    hull_scan_kernel                    one workgroup, tiles of 4096 labels: 16 tiles at max_out = 65 536 (the sparse test), 2 at the
                                        6240 labels of tests/test_gpu_hull.py.
    hull_fill_kernel                    1024 x 256 = 262 144 used slots (a label of height H takes H + 1): 128 x 2101 = 268 928 in
                                        test_hull_more_slots_than_one_trip_of_the_fill, in all four workspace states, with exact
                                        row room and with h * w; the four labels past the boundary are mostly empty levels.
    hull_chain_kernel                   HULL_MAX_CHAINS = 32 768 one-wave workgroups over 2 max_out: max_out > 16 384.  Four trips
                                        in test_hull_sparse_high_label_numbers, on one wave in consecutive trips: LDS path then
                                        register path, the reverse, LDS then a shorter LDS label, pixels then none, none then pixels.
                                        Its memory paths: 2101 levels (the fill test), 16 385 levels (test_hull_coordinate_limits
                                        [tall]); both passes in memory at 16 385 levels: test_hull_memory_passes_at_the_largest_height.
    hull_caliper_kernel                 HULL_MAX_GROUPS = 4096 x 4 waves = 16 384 labels: the same four trips.
    hull_pack (y << 15 | x)             x = 16384 and y = 16384: test_hull_coordinate_limits, also against hand-derived rectangles.
  spatial.hip.
    spatial_points_kernel               one workgroup, 256 droplets a step, `kept` carried: tables of 257 and 600, cut at 300, and
                                        with a capacity of 16 384: test_droplet_tables_longer_than_one_chunk.
    spatial_window_count_kernel         sized for 16 steps a thread, 1024 x 256 pixels a step: every window of more than 4096 pixels
                                        takes several steps (tests/test_gpu_spatial.py); past 4 194 304 pixels only their number
                                        grows.  Deliberately not reached.
    spatial_window_rows_kernel          4096 x 4 waves = 16 384 rows a trip, and h <= 16 384: no second trip exists.  h = 16 384:
                                        test_ripley_coordinate_limits (also the 64 trips of 256 rows of spatial_window_scan_kernel).
    spatial_sets_kernel                 4096 x 256 = 1 048 576 points of all sets: (1 + 999) x 1049 = 1 049 000 in
                                        test_ripley_sets_kernel_second_trip; the last simulation holds the boundary.
    spatial_eligible_kernel             one workgroup per set, 256 points a step: N = 1025 (tests/test_gpu_spatial.py), 4100 here.
    spatial_pairs_kernel                tiles of RIPLEY_TILE = 2048 points: N = 2049 and 4100 (second and third tile, the last of
                                        four points, coincident points across tiles) in test_ripley_second_and_third_lds_tile.  Grid
                                        max(1, 4096 // (1 + S)) workgroups of 4 i: ceil(N / 4) > 4096 // (1 + S) at N = 165, S = 99
                                        (2 trips) and N = 70, S = 999 (5 trips): test_ripley_later_trips_of_the_i_loop.  The set
                                        stride is max_points, not N: max_points = 16 384 over N = 0, 65, 300 in
                                        test_ripley_capacity_far_above_the_point_count and
                                        test_ripley_points_from_a_table_shorter_than_its_capacity.  Scan chunks of 64 bins:
                                        R = 63, 65, 127, 128, 255 in test_ripley_radii_around_the_scan_chunks.  Sides of 16 384:
                                        test_ripley_coordinate_limits.
  border.hip.
    border_init_kernel, border_merge_kernel, border_flatten_kernel   4096 x 256 = 1 048 576 pixels per image: n = 2 at 1100 x 960
                                        (1 056 000), a component across pixel 1 048 576 in both:
                                        test_border_planes_on_the_second_trip_of_two_images, and the weights bit for bit in
                                        test_border_weights_on_the_second_trip_of_two_images.
    border_col_kernel, border_row_kernel   one workgroup per tile, no loop over the grid.
  outlines.hip.  tests/test_gpu_outlines.py stops at 12 707 corners (13 tiles), 12 578 cracks (13 tiles) and 14 rounds.
    ol_init_kernel                      1024 x 256 = 262 144 words over 6 max_out: max_out > 43 690.  max_out = 65 536 (what the
                                        flow passes) over a canary-filled output: test_outlines_past_the_corner_grid.
    ol_census_kernel, ol_base_kernel    one workgroup per tile of 1024 corners, no loop over the grid: a second trip does not
                                        exist.  Tiles past 1024 and 2048 read tile_base entries of a later scan trip: the same tests
                                        as the crack scan.
    ol_scan_cracks_kernel (scan_plane, wave_ops.h, over the corner tiles)   1024 tiles = 1 048 576 corners a trip, `run` carried.  1034 tiles
                                        with ONE contour through all of them (1100 x 960):
                                        test_outlines_one_contour_longer_than_a_trip; 2067 and 2068 tiles, three trips:
                                        test_outlines_past_the_corner_grid; 1413 tiles at 1040 x 1388:
                                        test_label_outlines_batch_at_full_size.
    ol_successor_kernel                 8192 x 256 = 2 097 152 corners: 2 115 858 and 2 116 722 at 8200 x 257 and 600 x 3521, a
                                        label with cracks on both sides of that corner: test_outlines_past_the_corner_grid.
    ol_leader_kernel, ol_cut_kernel, ol_rank_kernel, ol_vertices_kernel   OL_MAX_GRID = 4096 x 256 = 1 048 576 cracks.  One contour
                                        of 1 057 102 cracks, so every jump of the later rounds crosses the trip boundary, 21 rounds;
                                        max_len = 2^20 (20 rounds) leaves the cycle longer than the windows, and the disagreement
                                        is the cut kernel's to find, with cracks on its second trip; max_len = length - 1 is the
                                        OL_LEN path at 21 rounds: test_outlines_one_contour_longer_than_a_trip.  264 992 contours
                                        of 4 cracks, 2665 of them on the second trip: test_outlines_more_contours_than_a_trip.
                                        Round counts 5 .. 30 on one small map, both parities of lead / rank / fin, jumps that
                                        wrap every cycle many times: test_outlines_every_round_count.
    ol_contour_count_kernel, ol_contours_kernel   one workgroup per tile of 1024 cracks of ROOM, no loop over the grid.  Their tile
                                        counts are what the contour scans read: below.
    ol_scan_contours_kernel (scan_plane over the crack tiles, twice) and tile_at[0 / 1] read back   1024 tiles = 1 048 576
                                        cracks of room.  1036 tiles, all in use, rooms cut inside the second trip (262 147
                                        contours, 1 048 578 vertices: mid-contour): test_outlines_more_contours_than_a_trip.
                                        1647 and 1651 tiles of room over 58 tiles of cracks (rooms_for(area, connected=False), as
                                        the flow asks): the second trip sums tiles past n, which ol_contour_count_kernel must have
                                        written as zero over a workspace of ones and a stale one:
                                        test_outlines_rooms_far_above_the_counts, and behind label_outlines_batch at 1040 x 1388
                                        (1128 tiles) with the shared workspace stale from the larger image before:
                                        test_label_outlines_batch_at_full_size.
    corner / (w + 1), the shoelace terms   sides of 16 384, a vertex at x = 16384 and one at y = 16384, also against hand-derived
                                        integers: test_outline_coordinate_limits.
    Deliberately not reached: corners near 2^29 (the most `where` packs beside its 3 low bits) need a label map of two gigabytes;
    a prefix past 2^31 in scan_plane needs as many cracks.

The fixtures of the hull, Ripley, border and outline tests are in tests/cap_fixtures.py, each with a premise that fails when it stops
reaching its loop; tests/test_droplet_edges_cpu.py runs the premises, and checks the mirrored caps against the sources, without a
device.  Timed once (host reference and device together, on the GPU machine): the sparse hull 0.24 s, the fill test 0.2 s per
state, the hull at the cap shapes 0.14 s, Ripley at N = 4100 0.24 s, S = 999 0.07 s, the two border tests 1.5 s together (most of it
border_weights_numpy, about 5 s on a slow host); everything else below 0.1 s.  The outline tests: one contour longer than a
trip 1.9 s (six runs on canaried buffers of 60 MB, and the followers of the serpentine and of the checkerboard, 0.4 s and
0.75 s, which every later test shares), past the corner grid 0.26 s and 0.22 s (their followers 0.2 s each), the batch at full
size 0.16 s, more contours than a trip 0.08 s, rooms far above the counts 0.05 s, every round count (28 runs) and the
coordinate limits 0.02 s each.

The label maps (tests/droplet_edge_fixtures.py:cap_labels) are the components of a blob mask: a few hundred droplets that
cross the 64-pixel seams, some of them the row where the second trip starts, and one in the last rows and columns.  Host
references at these shapes, timed on the CPU: label_props_numpy 0.25 s, overlap_table_numpy 0.03 s (0.2 s on
unique_pair_labels), the plain loops of tests/match_ref.py 0.5 s, offset_pairs and neighbor_columns on the 1500 x 1500 lattice
1.3 s -- the shapes the cap asks for are kept."""
import numpy as np
import pytest

from tests import cap_fixtures as cf
from tests import droplet_edge_fixtures as fx
from tests import hull_ref, neighbors_ref
from tests import spatial_ref
from tests.match_ref import overlap_table_ref
from tests.test_gpu_border import SIGMA, W0
from tests.test_gpu_border import run as border_run
from tests.test_gpu_hull import device_hull
from tests.test_gpu_match import assert_arrays_equal_host_path, device_overlap, host_table
from tests.test_gpu_neighbors import device_neighbors_arrays
from tests.test_gpu_outlines import FIXTURES as OUTLINE_FIXTURES
from tests.test_gpu_outlines import assert_equal as assert_outlines_equal
from tests.test_gpu_outlines import device_outlines, exact_rooms, ref_of
from tests.test_gpu_shape import NQ, assert_props_equal
from tests.test_gpu_spatial import assert_counts_equal_host, device_counts, device_points
from tests.test_match_cpu import kmax
from tests.test_shape_cpu import gray_plane
from tests.workspace_states import STATES, holds
from utils import droplet_hull as dh
from utils import droplet_neighbors as dn
from utils import droplet_outlines as do
from utils import droplet_shape as sh
from utils import spatial_stats as ss
from utils.border_weights import border_weights_numpy

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


# ---- hull.hip ----------------------------------------------------------------------------------------------------------------------

def assert_hull_rows(rows, want):
    """rows, want: int64 [5, max_out]."""
    for j, q in enumerate(dh.QUANTITIES):
        assert np.array_equal(rows[j], want[j]), (q, np.flatnonzero(rows[j] != want[j])[:5].tolist())


def host_rows(lab, max_out):
    ref = dh.label_hull_numpy(lab, max_out)
    return np.stack([ref[q] for q in dh.QUANTITIES])


def test_hull_sparse_high_label_numbers():
    """max_out = 65 536 on a 96 x 130 map whose fourteen labels carry numbers in all four trips of hull_chain_kernel and
    hull_caliper_kernel.  The hull depends on the pixel set alone: the expected rows are those of the same map numbered 1..14 (plain
    loops), at the high numbers; every other number keeps the zeros of hull_init_kernel, whose 327 680 words take a second trip."""
    compact, high, numbers = cf.hull_sparse_maps()
    max_out = cf.HULL_SPARSE_MAX_OUT
    cf.assert_hull_sparse_premise(high, max_out)
    want = cf.scatter_rows(hull_ref.label_hull_ref(compact, len(numbers)), numbers, max_out)
    assert (want[4, numbers - 1] >= 4).all() and np.count_nonzero(want[4]) == len(numbers)
    need = cf.rows_needed(high, max_out)
    rows, n_rows, _ = device_hull(high, max_out, max_rows=need)
    assert n_rows == need
    assert_hull_rows(rows, want)
    again, n_rows, _ = device_hull(high, max_out, max_rows=need, prefill=0xFF, state="ones")
    assert n_rows == need and again.tobytes() == rows.tobytes()


_columns = {}


def columns_rows():
    if not _columns:
        _columns["rows"] = host_rows(cf.hull_columns_map(), cf.HULL_COLUMNS)
        _columns["rows"].setflags(write=False)
    return _columns["rows"]


@pytest.mark.parametrize("state", STATES)
def test_hull_more_slots_than_one_trip_of_the_fill(state):
    """128 labels of 2101 corner levels: 268 928 used slots, so hull_fill_kernel comes round again; the last four labels lie
    beyond slot 262 144 and are mostly levels without a pixel, which the chains skip only where the fill reached them."""
    lab = cf.hull_columns_map()
    cf.assert_hull_columns_premise(lab)
    h, w = lab.shape
    want = columns_rows()
    assert all(tuple(want[:, k]) == cf.rect_integers(h, 1) for k in range(cf.HULL_COLUMNS))       # every hull is the 2100 x 1 rectangle
    stale = None
    if state == "stale":                                     # what the stage left at another geometry and capacity
        _, high, _ = cf.hull_sparse_maps()
        stale = device_hull(high, cf.HULL_SPARSE_MAX_OUT, max_rows=cf.rows_needed(high, cf.HULL_SPARSE_MAX_OUT))[2].u8.clone()
    exact = cf.HULL_COLUMNS * h
    for max_rows in (exact, h * w):
        rows, n_rows, ws = device_hull(lab, cf.HULL_COLUMNS, max_rows=max_rows, state=state, stale=stale)
        assert n_rows == exact and not holds(ws, state, stale)
        assert_hull_rows(rows, want)


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_label_hull_past_the_grid_cap(shape):
    """hull_extent_kernel and hull_rows_kernel share the frame of label_props_kernel: 8192 x 4 units a trip."""
    lab = fx.cap_labels(shape)[0]
    assert_reaches_the_second_trip(lab)
    k = kmax(lab)
    need = cf.rows_needed(lab, k)
    rows, n_rows, _ = device_hull(lab, k, max_rows=need, state="ones")
    assert n_rows == need
    assert_hull_rows(rows, host_rows(lab, k))


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_hull_coordinate_limits(name):
    """A vertex at x = 16384 and one at y = 16384: the largest values hull_pack holds, and the largest products of the calipers."""
    lab, hand = cf.hull_limit_maps()[name]
    h, w = lab.shape
    assert max(h, w) == 16384 and (lab[:, w - 1] > 0).any() and (lab[h - 1] > 0).any()
    if name == "tall":
        assert (lab[:, 0] == 1).all() and h + 1 > fx.HULL_LDS_POINTS        # 16 385 levels: the first chain pass in memory
    need = cf.rows_needed(lab, 2)
    rows, n_rows, _ = device_hull(lab, 2, max_rows=need, state="ones")
    assert n_rows == need
    assert_hull_rows(rows, host_rows(lab, 2))
    for k, ints in hand.items():
        assert tuple(int(v) for v in rows[:, k - 1]) == ints, k


def test_hull_memory_passes_at_the_largest_height():
    """16 385 levels with 2160 chunk vertices on the left side: both chain passes run in memory, up to y = 16384."""
    lab = cf.hull_tall_parabolas()
    c, kept = cf.chunk_chain_points(cf.left_candidates(lab, 1), 1)
    assert lab.shape[0] == 16384 and c == 257 and kept > fx.HULL_LDS_POINTS
    rows, n_rows, _ = device_hull(lab, 1, max_rows=16384, state="ones")
    assert n_rows == 16384
    assert_hull_rows(rows, host_rows(lab, 1))


# ---- spatial.hip -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("windowed", [False, True], ids=["null", "holes"])
@pytest.mark.parametrize("N", cf.RIPLEY_TILE_COUNTS)
def test_ripley_second_and_third_lds_tile(N, windowed):
    py, px, win = cf.ripley_tile_points(N, windowed)
    cf.assert_ripley_tiles_premise(N, py, px)
    n, pairs, pairs_all = assert_counts_equal_host(py, px, *cf.RIPLEY_SHAPE, 64, 1, 17, win)
    assert pairs_all[0][0] >= 2 * len(cf.coincident_pairs(N)) and pairs_all[0][64] > N       # c = 0 pairs: only t0 + j != i tells i from j


@pytest.mark.parametrize("N,S,trips", [(165, 99, 2), (70, 999, 5)])
def test_ripley_later_trips_of_the_i_loop(N, S, trips):
    """165 points at the flow's S = 99: 40 workgroups, and a second trip in which workgroup 1 has one active wave.  70 points at
    S = 999, the most the ABI takes: 4 workgroups, five trips, the last of 6 i."""
    groups, got = cf.assert_second_i_trip(N, S)
    assert (groups, got) == ({99: 40, 999: 4}[S], trips) and N % 4 != 0
    h, w = 96, 130
    win = cf.ripley_holes_window(h, w)
    py, px = ss.simulated_points(50 + N, 0, N, h, w, win)
    n, pairs, pairs_all = assert_counts_equal_host(py, px, h, w, 16, S, 4321, win)
    assert len({tuple(r) for r in pairs_all[1:].tolist()}) > S // 2


@pytest.mark.parametrize("N", [0, 65, 300])
def test_ripley_capacity_far_above_the_point_count(N):
    """max_points = 16 384 as in the flow: the set stride is the capacity, not N, and most workgroups start past N."""
    h, w = 96, 130
    cap = cf.RIPLEY_CAPACITY
    assert cap >= 16384 > 4 * N and cf.pair_grid(cap, 3) * 4 > N
    for win in (None, cf.ripley_holes_window(h, w)):
        py, px = ss.simulated_points(60 + N, 0, N, h, w, win)
        want = ss.ripley_counts_numpy(py, px, h, w, 16, 3, 9, win)
        got = device_counts(py, px, h, w, 16, 3, 9, win, max_points=cap)[:3]
        for name, g, v in zip(("n", "pairs", "pairs_all"), got, want):
            assert np.array_equal(g, v), (name, np.argwhere(g != v)[:5].tolist())
        assert N == 0 or (want[2][1:, 16] > 0).all()


def test_ripley_points_from_a_table_shorter_than_its_capacity():
    h, w, cap = 96, 130, cf.RIPLEY_CAPACITY
    area, sy, sx, window = spatial_ref.random_case(h, w, 70, "holes", seed=5)
    want_py, want_px, info = ss.droplet_points(area, sy, sx, h, w, window)
    py, px, got = device_points(area, sy, sx, h, w, window, max_points=cap)
    assert np.array_equal(py, want_py) and np.array_equal(px, want_px)
    assert got.tolist() == [info["N"], info["n_dropped"], info["A"], 0] and 0 < info["n_dropped"] < 70
    want = ss.ripley_counts_numpy(py, px, h, w, 16, 3, 9, window)
    got = device_counts(py, px, h, w, 16, 3, 9, window, max_points=cap)[:3]
    assert all(np.array_equal(g, v) for g, v in zip(got, want))


@pytest.mark.parametrize("k,cap", [(257, 257), (600, 600), (600, 300), (600, cf.RIPLEY_CAPACITY)])
def test_droplet_tables_longer_than_one_chunk(k, cap):
    """spatial_points_kernel walks the table 256 droplets at a time and carries the number kept so far; max_points = 300 cuts the
    table inside its second chunk (the canaries past entry 300 are checked in device_points)."""
    h, w = 96, 130
    area, sy, sx, window = cf.long_table(k)
    cf.assert_table_chunks_premise(area, sy, sx, h, w, window, cap)
    n = min(k, cap)
    want_py, want_px, info = ss.droplet_points(area[:n], sy[:n], sx[:n], h, w, window)
    py, px, got = device_points(area, sy, sx, h, w, window, max_points=cap)
    assert np.array_equal(py, want_py) and np.array_equal(px, want_px)                   # table order
    assert got.tolist() == [info["N"], info["n_dropped"], info["A"], int(k > cap)]
    assert info["N"] + info["n_dropped"] == n and info["n_dropped"] > 0


@pytest.mark.parametrize("R", [63, 65, 127, 128, 255])
def test_ripley_radii_around_the_scan_chunks(R):
    """The scan of a wave's bins runs in chunks of 64 and stops at the first chunk that starts past R."""
    h, w = cf.RIPLEY_SHAPE
    assert (R + 1) % 64 in (0, 1, 2) and R not in (64, 256)
    win = cf.ripley_holes_window(h, w)
    py, px = ss.simulated_points(70 + R, 0, 65, h, w, win)
    n, pairs, pairs_all = assert_counts_equal_host(py, px, h, w, R, 1, 5, win)
    assert pairs_all[:, R].sum() > pairs_all[:, R - 1].sum() > pairs_all[:, R // 2].sum() > 0         # the last bin is in use


def test_ripley_sets_kernel_second_trip():
    """S = 999 and N = 1049: 1 049 000 points for spatial_sets_kernel against 1 048 576 a trip; the points across that index are
    those of the last simulation from its point 625 on.  The full host reference takes a quarter of a minute, so the observed
    pattern, the first two and the last three simulations are compared, each a host call of its own on simulated_points."""
    c = cf.RIPLEY_SETS_CASE
    S, N, R, h, w, seed = (c[q] for q in ("S", "N", "R", "h", "w", "seed"))
    cf.assert_ripley_sets_premise(S, N)
    py, px = ss.simulated_points(77, 0, N, h, w)
    n, pairs, pairs_all, _ = device_counts(py, px, h, w, R, S, seed)
    for s in (-1,) + cf.RIPLEY_SETS_CHECKED:
        qy, qx = (py, px) if s < 0 else ss.simulated_points(seed, s, N, h, w)
        want = ss.ripley_counts_numpy(qy, qx, h, w, R, 0, seed)
        for name, g, v in zip(("n", "pairs", "pairs_all"), (n, pairs, pairs_all), want):
            assert np.array_equal(g[s + 1], v[0]), (s, name, g[s + 1].tolist(), v[0].tolist())
    assert (n[:, 0] == N).all() and (pairs_all[:, R] > 0).all() and (pairs_all[:, R] >= pairs[:, R]).all()


@pytest.mark.parametrize("hw", [(16384, 2), (2, 16384)], ids=lambda v: "{}x{}".format(*v))
def test_ripley_coordinate_limits(hw):
    """The largest sides: packed coordinates of 16 383, squared differences of 16 383^2, m * m at the frame."""
    h, w = hw
    py, px = cf.ripley_limit_points(h, w)
    assert max(py) == h - 1 and max(px) == w - 1 and min(py) == min(px) == 0 and max(h, w) == 16384
    for win in (None, np.ones((h, w), np.uint8)):
        n, pairs, pairs_all = assert_counts_equal_host(py, px, h, w, 16, 3, 11, win)
        assert pairs_all[0][16] >= 8 and pairs_all[0][0] == 0


# ---- border.hip ------------------------------------------------------------------------------------------------------------------

_border = {}


def border_reference():
    if not _border:
        out = border_weights_numpy(cf.border_masks(), W0, SIGMA, cf.BORDER_RADIUS, planes=True)
        for v in out:
            v.setflags(write=False)
        _border["ref"] = out
    return _border["ref"]


def border_device():
    if not _border.get("dev"):
        _border["dev"] = border_run(cf.border_masks().copy(), cf.BORDER_RADIUS, state="ones")[:3]
    return _border["dev"]


def test_border_planes_on_the_second_trip_of_two_images():
    """n = 2 at 1100 x 960: border_init / merge / flatten come round again from pixel 1 048 576 (row 1092, column 256), where
    each mask holds a component on both sides; the second image tells a trip that forgot its image's base."""
    masks = cf.border_masks()
    assert cf.assert_border_premise(masks) == 1056000
    _, n1, n2 = border_reference()
    _, d1, d2 = border_device()                              # outputs and workspace between canaries (border_run)
    for i in range(2):
        assert np.array_equal(d1[i], n1[i]), (i, np.argwhere(d1[i] != n1[i])[:5].tolist())
        assert np.array_equal(d2[i], n2[i]), (i, np.argwhere(d2[i] != n2[i])[:5].tolist())
    y, x = divmod(fx.BORDER_PIXELS_PER_TRIP, masks.shape[2])
    assert (n2[:, y - 8:y + 9, x - 16:x + 17] <= cf.BORDER_RADIUS ** 2).any(axis=(1, 2)).all()   # border terms around the boundary


def test_border_weights_on_the_second_trip_of_two_images():
    masks = cf.border_masks()
    cf.assert_border_premise(masks)
    nw, _, _ = border_reference()
    wt, _, _ = border_device()
    diff = wt.view(np.uint32) != nw.view(np.uint32)
    print(f"\n border weights, 2 x 1100 x 960 at R {cf.BORDER_RADIUS}: {int(diff.sum())} of {int((nw > 1).sum())} weights above 1 differ from "
          f"the host path; largest gap {float(np.abs(wt.astype(np.float64) - nw).max()):.3e}")
    assert not diff.any(), np.argwhere(diff)[:5].tolist()


# ---- outlines.hip ----------------------------------------------------------------------------------------------------------------
# Every comparison is integer for integer and vertex for vertex against the sequential follower (cf.outline_ref: once per fixture,
# read-only); device_outlines puts the label map, every output and the workspace between canaries.

OQ, OF = do.QUANTITIES, do.CONTOUR_FIELDS


def outline_bytes(rec):
    return b"".join(rec[part][k].tobytes() for part in ("rows", "contours") for k in rec[part]) + rec["x"].tobytes() + rec["y"].tobytes()


def outline_counts_of(ref):
    r = exact_rooms(ref)
    return [r["max_cracks"], r["max_contours"], r["max_vertices"], 0]


def assert_nothing_listed(rec, cont, vx, vy):
    assert cont.untouched() and vx.untouched() and vy.untouched() and not any(rec["rows"][q].any() for q in OQ)


def assert_prefix_listed(rec, ref, nc, nv):
    """The per-label rows are complete; the table and the vertex lists hold what the follower lists first."""
    for q in OQ:
        assert np.array_equal(rec["rows"][q], ref["rows"][q]), q
    assert (len(rec["contours"]["label"]), len(rec["x"]), len(rec["y"])) == (nc, nv, nv)
    for f in OF:
        assert np.array_equal(rec["contours"][f], ref["contours"][f][:nc]), f
    assert np.array_equal(rec["x"], ref["x"][:nv]) and np.array_equal(rec["y"], ref["y"][:nv])


def test_outlines_one_contour_longer_than_a_trip():
    """1100 x 960, one contour of 1 057 102 cracks through 1034 corner tiles: the crack scan's second trip, and 21 leader and 21
    rank rounds whose jumps cross crack 1 048 576 in both directions.  The stale workspace is what the checkerboard left."""
    lab, ref = cf.outline_ref("serpentine")
    assert cf.assert_outline_serpentine_premise(lab, ref) == (1058061, 1034, 1057102, 1, 2202, 21)
    rooms, A = exact_rooms(ref), int(lab.sum())
    board, board_ref = cf.outline_ref("checkerboard")
    stale = device_outlines(board, 3, exact_rooms(board_ref))[2][0].u8.clone()
    runs = []
    for state in ("ones", "stale"):
        rec, needed, (ws, *_) = device_outlines(lab, 1, rooms, state=state, stale=stale)
        assert needed.tolist() == [1057102, 1, 2202, 0] and not holds(ws, state, stale)
        assert_outlines_equal(rec, ref)
        assert rec["contours"]["length"].tolist() == [2 * A + 2] and rec["contours"]["S2"].tolist() == [2 * A]
        runs.append(outline_bytes(rec))
    assert runs[0] == runs[1]
    # 2^20: 20 rounds, the cycle is longer than the windows (ol_cut_kernel finds it); length - 1: 21 rounds, the OL_LEN path
    for short, rounds in ((1 << 20, 20), (rooms["max_len"] - 1, 21)):
        assert cf.outline_rounds(short) == rounds and short < rooms["max_len"]
        rec, needed, (_, cont, vx, vy) = device_outlines(lab, 1, {**rooms, "max_len": short}, state="ones")
        assert needed.tolist() == [1057102, 0, 0, 1], short
        assert_nothing_listed(rec, cont, vx, vy)
    rec, needed, (_, cont, vx, vy) = device_outlines(lab, 1, {**rooms, "max_cracks": 1 << 20}, state="ones")      # one trip of room
    assert needed.tolist() == [1057102, 0, 0, 0]
    assert_nothing_listed(rec, cont, vx, vy)


def test_outlines_more_contours_than_a_trip():
    """728 x 728, 264 992 one-pixel contours in 1036 crack tiles and one trip of corners: the crack-side loops and both contour
    scans on their second trip, alone."""
    lab, ref = cf.outline_ref("checkerboard")
    assert cf.assert_outline_checkerboard_premise(lab, ref)[:5] == (531441, 1059968, 264992, 1059968, 1036)
    rooms = exact_rooms(ref)
    rec, needed, _ = device_outlines(lab, 3, rooms, state="ones")
    assert needed.tolist() == [1059968, 264992, 1059968, 0]
    assert_outlines_equal(rec, ref)
    c = rec["contours"]                                      # without the follower: pixel by pixel in raster order
    rr, cc = np.nonzero(lab)
    assert (c["length"] == 4).all() and (c["nv"] == 4).all() and (c["S2"] == 2).all() and np.array_equal(c["first"], 4 * np.arange(264992))
    assert np.array_equal(c["label"], 1 + (rr // 100) % 3)
    assert np.array_equal(rec["x"].reshape(-1, 4), cc[:, None] + np.array([0, 1, 1, 0])) and np.array_equal(rec["y"].reshape(-1, 4), rr[:, None] + np.array([0, 0, 1, 1]))
    area = np.bincount(lab.ravel(), minlength=4)[1:]
    assert np.array_equal(rec["rows"]["E"], 4 * area) and np.array_equal(rec["rows"]["no"], area) and not rec["rows"]["nh"].any()
    cut = {**rooms, "max_contours": (1 << 18) + 3, "max_vertices": (1 << 20) + 2}        # inside the second trip, mid-contour
    assert cut["max_vertices"] % 4 == 2 and cut["max_vertices"] < 4 * cut["max_contours"]
    rec, needed, _ = device_outlines(lab, 3, cut, state="ones")                          # the canaries held
    assert needed.tolist() == [1059968, 264992, 1059968, 0]
    assert_prefix_listed(rec, ref, cut["max_contours"], cut["max_vertices"])


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_outlines_past_the_corner_grid(shape):
    """More than 8192 x 256 corners, three trips of the crack scan; then max_out = 65 536 as the flow passes it: 393 216 output
    words, the second trip of ol_init_kernel, over an output that held the canary pattern."""
    lab, ref = cf.outline_ref("{}x{}".format(*shape))
    cf.assert_outline_corner_grid_premise(lab, ref)
    k, rooms = kmax(lab), exact_rooms(ref)
    rec, needed, _ = device_outlines(lab, k, rooms, state="ones")
    assert needed.tolist() == outline_counts_of(ref)
    assert_outlines_equal(rec, ref)
    big = 65536
    assert len(OQ) * big > fx.OUTLINE_INIT_WORDS_PER_TRIP
    rec, needed, _ = device_outlines(lab, big, rooms, state="ones")
    assert needed.tolist() == outline_counts_of(ref)
    assert all(rec["rows"][q].shape == (big,) and not rec["rows"][q][k:].any() for q in OQ)      # zeros, not the canary
    rec["rows"] = {q: rec["rows"][q][:k] for q in OQ}
    assert_outlines_equal(rec, ref)


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_outlines_rooms_far_above_the_counts(shape):
    """rooms_for(area, connected=False), as the flow asks: about 1.69 M cracks of room over 58 tiles of cracks, so the contour
    scans take a second trip over tiles past n, and 21 rounds run over contours of at most 1354 cracks."""
    from unet_dc_segmentation_amd.outlines import rooms_for
    lab, ref = cf.outline_ref("{}x{}".format(*shape))
    k = kmax(lab)
    rooms = rooms_for(np.bincount(lab.ravel(), minlength=k + 1)[1:], connected=False)
    counts = outline_counts_of(ref)
    assert cf.tiles(rooms["max_cracks"]) > fx.OUTLINE_SCAN_TILES_PER_TRIP > cf.tiles(counts[0])
    assert cf.outline_rounds(rooms["max_len"]) == 21 and exact_rooms(ref)["max_len"] <= 1354
    other = fx.CAP_SHAPES[1 - fx.CAP_SHAPES.index(shape)]    # stale: what the stage left at the other shape with exact rooms
    other_lab, other_ref = cf.outline_ref("{}x{}".format(*other))
    stale = device_outlines(other_lab, kmax(other_lab), exact_rooms(other_ref))[2][0].u8.clone()
    runs = []
    for state in ("ones", "stale"):
        rec, needed, (ws, *_) = device_outlines(lab, k, rooms, state=state, stale=stale)
        assert needed.tolist() == counts and not holds(ws, state, stale)
        assert_outlines_equal(rec, ref)
        runs.append(outline_bytes(rec))
    assert runs[0] == runs[1]


def test_outlines_every_round_count():
    """max_len = 2^r for every r from the fewest rounds that hold the longest contour to 30, then 2^29 + 1 and 2^30: both parities
    of lead / rank / fin, jumps that wrap every cycle many times.  One record, the same bytes, at every count."""
    name = "37x53 random"
    lab, ref = OUTLINE_FIXTURES[name], ref_of(name)
    rooms = exact_rooms(ref)
    L = rooms["max_len"]
    r0 = cf.outline_rounds(L)
    assert 1 << r0 >= L > 1 << (r0 - 1) and 4 < r0 < 15
    lens = [1 << r for r in range(r0, 31)] + [(1 << 29) + 1, 1 << 30]
    assert [cf.outline_rounds(v) for v in lens] == list(range(r0, 31)) + [30, 30]
    first = None
    for max_len in lens:
        rec, needed, _ = device_outlines(lab, 3, {**rooms, "max_len": max_len}, state="a5")
        assert needed.tolist() == outline_counts_of(ref), max_len
        assert_outlines_equal(rec, ref)
        first = outline_bytes(rec) if first is None else first
        assert outline_bytes(rec) == first, max_len


@pytest.mark.parametrize("name", ["tall", "wide"])
def test_outline_coordinate_limits(name):
    """Sides of 16 384: a bar with a vertex on the last lattice line, two small contours at the far corner."""
    lab, hand = cf.outline_limit_maps()[name]
    ref = cf.outline_ref(name)[1]
    cf.assert_outline_limit_premise(name, lab, ref, hand)
    rec, needed, _ = device_outlines(lab, 2, exact_rooms(ref), state="ones")
    assert needed.tolist() == outline_counts_of(ref)
    assert_outlines_equal(rec, ref)
    for k, ints in hand.items():
        assert tuple(int(rec["rows"][q][k - 1]) for q in OQ) == ints, k
    assert int(rec["y" if name == "tall" else "x"].max()) == 16384


def test_label_outlines_batch_at_full_size():
    """label_outlines_batch with the rooms it computes itself (connected=False) on a 1040 x 1388 blob map (1 154 852 cracks of
    room: second trips of the crack scan and of both contour scans, 21 rounds), the 96 x 130 serpentine in the workspace the larger
    image left, and 600 x 3521: three launches, no retry."""
    import torch
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.outlines import label_outlines_batch, rooms_for
    small = "96x130 serpentine"
    cases = [cf.outline_ref("blobs"), (OUTLINE_FIXTURES[small], ref_of(small)), cf.outline_ref("600x3521")]
    areas = [np.bincount(lab.ravel(), minlength=kmax(lab) + 1)[1:] for lab, _ in cases]
    rooms = [rooms_for(a, connected=False) for a in areas]
    assert rooms[0]["max_cracks"] == 4 * int((cases[0][0] > 0).sum()) == 1154852 > fx.OUTLINE_CRACKS_PER_TRIP
    need = [_lib.load().unetdc_label_outlines_workspace(*lab.shape, len(a), r["max_cracks"]) for (lab, _), a, r in zip(cases, areas, rooms)]
    assert need[0] > need[1] > 0 and need[2] > need[0]       # the small image runs in a workspace stale from a larger one
    labs = [torch.from_numpy(lab.copy()).cuda() for lab, _ in cases]
    calls = []
    real = _lib.call
    try:
        _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        recs = label_outlines_batch(labs, areas, connected=False)
    finally:
        _lib.call = real
    assert calls == ["unetdc_label_outlines"] * 3            # no image ran again
    for rec, (lab, ref), area in zip(recs, cases, areas):
        assert_outlines_equal(rec, ref)
        cols, want = do.outline_columns(rec, area), do.outline_columns(ref, area)
        assert list(cols) == list(want) and all(cols[q].tobytes() == want[q].tobytes() for q in want)
