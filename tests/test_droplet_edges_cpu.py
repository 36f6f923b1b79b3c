"""CPU: what the inputs and host-side rules of the workspace-state, grid-cap and C-ABI density tests are for
(tests/workspace_states.py, tests/droplet_edge_fixtures.py), checked without a device."""
import pathlib
import re

import numpy as np
import pytest
import torch

from tests import cap_fixtures as cf
from tests import droplet_edge_fixtures as fx
from tests import hull_ref, spatial_ref
from tests import workspace_states as wss
from tests.image_canaries import CANARY, Canaried
from tests.match_ref import overlap_table_ref
from tests.test_density_cpu import cell_image
from tests.test_hull_cpu import known_shapes
from tests.test_match_cpu import kmax
from utils import density as hd
from utils import droplet_hull as dh
from utils import droplet_match as dm
from utils import droplet_outlines as do
from utils import droplet_shape as sh
from utils import spatial_stats as ss


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_fit_bytes_cuts_or_repeats():
    src = torch.arange(10, dtype=torch.uint8)
    assert wss.fit_bytes(src, 4).tolist() == [0, 1, 2, 3] and wss.fit_bytes(src, 10).tolist() == list(range(10))
    assert wss.fit_bytes(src, 23).tolist() == (list(range(10)) * 3)[:23] and wss.fit_bytes(src, 0).numel() == 0


@pytest.mark.parametrize("state", wss.STATES)
def test_prepare_fills_the_view_and_nothing_else(state):
    stale = torch.arange(700, dtype=torch.int32).to(torch.uint8)
    ws = wss.prepare(Canaried(1000, device="cpu"), state, stale)
    ws.check()
    assert wss.holds(ws, state, stale)
    want = {"zero": 0, "ones": 255, "a5": 0xA5}.get(state)
    assert bool((ws.u8 == want).all()) if want is not None else ws.u8[:700].tolist() == stale.tolist() and ws.u8[700:].tolist() == stale[:300].tolist()
    ws.u8[999] ^= 1
    assert not wss.holds(ws, state, stale)
    assert bool((ws.buf[:ws.start] == CANARY).all())


def test_droplet_table_is_the_ccl_stats_table():
    m = np.zeros((6, 9), np.uint8)
    m[0, 7:9] = m[2:4, 1:3] = m[5, 0] = 1
    a, sy, sx = wss.droplet_table(m)
    assert a.dtype == np.int32 and a.tolist() == [2, 4, 1] and sy.tolist() == [0, 10, 5] and sx.tolist() == [15, 6, 0]


def test_unit_numbering_and_the_second_trip_predicate():
    assert fx.WAVE_UNITS_PER_TRIP == 32768
    assert fx.unit_of(0, 63, 257) == 0 and fx.unit_of(0, 64, 257) == 1 and fx.unit_of(0, 256, 257) == 4 and fx.unit_of(1, 0, 257) == 5
    lab = np.zeros((8, 130), np.int32)                         # 3 units per row
    lab[2, 60:70] = 1                                          # units 6 and 7
    lab[5, 129] = 2                                            # unit 17, the one-pixel unit of row 5
    lab[7, 0] = 3                                              # unit 21
    assert fx.labels_past_unit(lab, 7).tolist() == [1, 2, 3] and fx.labels_before_unit(lab, 7).tolist() == [1]
    assert fx.labels_past_unit(lab, 8).tolist() == [2, 3] and fx.labels_past_unit(lab, 18).tolist() == [3]
    assert fx.labels_past_unit(lab, 22).tolist() == [] and fx.labels_before_unit(lab, 6).tolist() == []
    assert fx.labels_past_unit(lab).tolist() == []             # nothing here reaches unit 32 768


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cap_label_maps_hold_what_they_are_for(shape):
    h, w = shape
    chunks = (w + 63) // 64
    assert w % 64 == 1 and h * chunks > fx.WAVE_UNITS_PER_TRIP                  # the last unit of a row holds one pixel
    assert (h, chunks, h * chunks) in ((8200, 5, 41000), (600, 56, 33600))
    assert 1 << 21 < h * w <= 1 << 22                                            # max_pairs = h * w: a sort of 2^22 entries
    row = fx.WAVE_UNITS_PER_TRIP // chunks                                       # the row in which the second trip starts
    for lab in fx.cap_labels(shape):
        k = kmax(lab)
        assert lab.dtype == np.int32 and 200 <= k <= 999 and np.array_equal(np.unique(lab), np.arange(k + 1))
        late, early = fx.labels_past_unit(lab), fx.labels_before_unit(lab)
        assert len(late) >= 10 and len(np.intersect1d(late, early)) >= 1
        assert (lab[row] > 0).any() and ((lab[:, 63] == lab[:, 64]) & (lab[:, 63] > 0)).any()
        assert lab[h - 1, w - 1] > 0 and (lab[h - 3:, w - 3:] == lab[h - 1, w - 1]).all()    # the corner droplet
    A, B = fx.cap_labels(shape)
    table = list(zip(*(v.tolist() for v in dm.overlap_table_numpy(A, B, kmax(A), kmax(B)))))
    assert 200 <= len(table) <= 999                                              # "a few hundred pairs"
    assert table == overlap_table_ref(A.tolist(), B.tolist(), kmax(A), kmax(B))  # the vectorised host path and the plain loops


PAIR_COUNTS = (4095, 4096, 4097, 8191, 8192, 8193, 12289)     # around one, two and three sort chunks


def pow2_at_least(v):
    return 1 << max(int(v) - 1, 0).bit_length()


@pytest.mark.parametrize("E", PAIR_COUNTS)
def test_pair_count_labels_hold_exactly_that_many_pairs(E):
    assert fx.PAIR_SORT_CHUNK == 4096 and fx.PAIR_SHAPE == (96, 256)
    a, b, n = fx.pair_count_pairs(E)
    assert len(a) == E and len(set(zip(a.tolist(), b.tolist()))) == E            # the construction: E distinct keys
    assert np.bincount(a)[1:-1].min() == fx.PAIR_B_PER_A                          # several b per a (the last a may have fewer)
    assert np.bincount(b, minlength=fx.PAIR_B_LABELS + 1)[1:].min() >= 50         # ... and many a per b: both halves of the key order
    assert (n == 2).sum() > E // 4 and (n == 3).sum() > E // 40 and n.min() == 1
    for shape in (fx.PAIR_SHAPE, (512, 512)):
        A, B = fx.pair_count_labels(E, shape)
        assert A.dtype == B.dtype == np.int32 and A.shape == B.shape == shape
        got = dm.overlap_table_numpy(A, B, kmax(A), kmax(B))
        assert all(np.array_equal(x, y) for x, y in zip(got, (a, b, n)))          # the host path finds what was put there
        assert kmax(A) == (E - 1) // fx.PAIR_B_PER_A + 1 and kmax(B) == fx.PAIR_B_LABELS
        assert ((A > 0) & (B == 0)).sum() > 100 and ((A == 0) & (B > 0)).sum() > 100      # labels that meet background only
        # the pixels of a pair with several lie apart: in different 64-pixel units, so each is an insert of its own
        key = (A.astype(np.int64) << 32 | B)[(A > 0) & (B > 0)]
        yy, xx = np.nonzero((A > 0) & (B > 0))
        units = np.unique(np.stack([key, fx.unit_of(yy, xx, shape[1])]), axis=1)
        assert (np.unique(units[0], return_counts=True)[1] >= 2).sum() > E // 4
    assert 512 * 512 >= 1 << 18                                                   # a capacity of 2^18 is not cut to h * w there
    h, w = fx.PAIR_SHAPE
    # the network of a tight capacity: one chunk, two, four
    assert pow2_at_least(E) == {4095: 4096, 4096: 4096, 4097: 8192, 8191: 8192, 8192: 8192, 8193: 16384, 12289: 16384}[E]
    assert E - 1 <= h * w and pow2_at_least(h * w) == 32768


def test_the_pair_counts_sit_on_both_sides_of_every_chunk_multiple():
    c = fx.PAIR_SORT_CHUNK
    assert [E for E in PAIR_COUNTS if E <= c] == [4095, 4096] and [E for E in PAIR_COUNTS if c < E <= 2 * c] == [4097, 8191, 8192]
    assert [E for E in PAIR_COUNTS if 2 * c < E <= 4 * c] == [8193, 12289] and 12289 == 3 * c + 1
    from unet_dc_segmentation_amd import droplets
    assert droplets.PAIR_ROOM == 4 * c                                            # what production launches with: four chunks


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unique_pair_labels_make_every_pixel_a_pair(shape):
    h, w = shape
    A, B = fx.unique_pair_labels(shape)
    assert A.dtype == B.dtype == np.int32 and np.array_equal(np.sort(A.ravel()), np.arange(1, h * w + 1))
    assert not np.array_equal(A.ravel(), np.arange(1, h * w + 1)) and np.array_equal(B.ravel(), np.arange(h * w) % 5 + 1)
    a, b, n = dm.overlap_table_numpy(A, B, h * w, 5)
    assert len(a) == h * w > 1 << 21 and pow2_at_least(h * w) == 1 << 22          # 2^21 compare-exchanges a pass: 4096 x 256 twice
    assert h * w > fx.PAIR_GRID_PER_TRIP == 524288 and (n == 1).all()
    assert np.array_equal(a, np.arange(1, h * w + 1)) and np.array_equal(b[A.ravel() - 1], B.ravel())


def test_expected_rows_layout_for_a_large_capacity():
    from tests.test_gpu_shape import NQ, expected_rows
    lab = fx.few_dozen_labels()
    k = kmax(lab)
    assert 24 <= k <= 100 and NQ * 20000 > 1024 * 256                            # past label_props_init_kernel's grid cap
    gray = np.random.default_rng(1).integers(0, 256, lab.shape).astype(np.uint8)
    for g in (None, gray):
        rows = expected_rows(lab, g, 20000)
        assert rows.shape == (NQ, 20000) and rows.dtype == np.int64
        assert np.array_equal(rows[:, k:], fx.initial_rows(NQ, 20000 - k, sh.QUANTITIES, sh.MIN_INIT, sh.MAX_INIT))
        p = sh.label_props_numpy(lab, g)
        assert np.array_equal(rows[sh.QUANTITIES.index("Syy"), :k], p["Syy"]) and (rows[sh.QUANTITIES.index("max_y"), :k] >= 0).all()
        assert (rows[10:, :k] == fx.initial_rows(4, k, sh.QUANTITIES[10:], sh.MIN_INIT, sh.MAX_INIT)).all() == (g is None)
    init = fx.initial_rows(NQ, 3, sh.QUANTITIES, sh.MIN_INIT, sh.MAX_INIT)
    assert init[:, 0].tolist() == [0, 0, 0, 2 ** 63 - 1, 2 ** 63 - 1, -1, -1, 0, 0, 0, 0, 0, 2 ** 63 - 1, -1]


def test_ring_rule_on_a_truncated_table():
    roi = np.zeros((30, 30), np.uint8)
    roi[10, 10:21] = 1                                                           # centroid (10, 15), largest distance 5
    area = np.array([1, 2, 1, 1], np.int32)
    sy = np.array([10, 20, 10, 10], np.int64)
    sx = np.array([16, 37, 15, 20], np.int64)                                    # distances 1, 3.5, 0 (no ring), 5
    assert hd.roi_centroid(roi)[:2] == (15, 10)
    assert fx.ring_counts_of_table(area, sy, sx, 4, roi, 5).tolist() == [1, 0, 0, 1, 1]
    assert fx.ring_counts_of_table(area, sy, sx, 3, roi, 5).tolist() == [1, 0, 0, 1, 0]
    assert fx.ring_counts_of_table(area, sy, sx, 1, roi, 5).tolist() == [1, 0, 0, 0, 0]
    assert fx.ring_counts_of_table(area, sy, sx, 0, roi, 5).tolist() == [0] * 5
    rgb, mask = cell_image(96, 130, 11)
    table = wss.droplet_table(mask)
    full = hd.density_maps(rgb, mask, 10, 21)
    assert np.array_equal(fx.ring_counts_of_table(*table, len(table[0]), full["roi"], 10), full["ring_counts"])


def test_bound_case_puts_droplets_on_exact_ring_bounds():
    rgb, mask, rings, counts = fx.bound_case()
    r = hd.density_maps(rgb, mask, fx.BOUND_LAYERS, 21)
    assert (r["threshold"], r["cx"], r["cy"], r["roi_area"], r["max_ring_distance"]) == (0, 80, 60, 121 * 161, 100.0)
    bounds = np.linspace(0, r["max_ring_distance"], fx.BOUND_LAYERS + 1)
    assert bounds.tolist() == [10.0 * i for i in range(11)]
    area, sy, sx = wss.droplet_table(mask)
    d = np.sqrt((sx / area - 80) ** 2 + (sy / area - 60) ** 2)
    assert len(d) == len(fx.BOUND_DROPLETS) and sorted(d.tolist()) == sorted(v for _, v, _ in fx.BOUND_DROPLETS)
    on_bound = np.isin(d, bounds)
    assert on_bound.sum() == len(d) - 1                                          # all but the droplet at distance 31
    assert hd.ring_of(bounds, d).tolist() == rings                               # lower ring on a bound, none at d = 0
    assert rings.count(-1) == 1 and np.array_equal(r["ring_counts"], counts) and counts.tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 0, 1]
    assert r["roi"][60, 80] == 1 and r["ring"][60, 80] == 0 and r["ring"][60, 90] == 1 and r["ring"][60, 91] == 2 and r["ring"][0, 0] == 10


# ---- the caps of hull.hip, spatial.hip and border.hip, and the fixtures of tests/cap_fixtures.py that pass them ---------------------

CSRC = pathlib.Path(__file__).resolve().parent.parent / "unet_dc_segmentation_amd" / "csrc"


def constexpr_int(source, name):
    """The value of `constexpr int NAME = <integer expression>;` in a source text (digits, shifts, + - * / and brackets only)."""
    m = re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([0-9()<>+\-*/ ]+)[,;]", source)
    assert m, name
    return int(eval(m.group(1).replace("/", "//"), {"__builtins__": {}}))


def test_cap_mirrors_equal_the_sources():
    hull, spatial, border = ((CSRC / f).read_text() for f in ("hull.hip", "spatial.hip", "border.hip"))
    for name in ("HULL_MAX_GROUPS", "HULL_MAX_CHAINS", "HULL_LDS_POINTS"):
        assert constexpr_int(hull, name) == getattr(fx, name), name
    assert constexpr_int(spatial, "RIPLEY_TILE") == fx.RIPLEY_TILE == 2048
    assert (fx.HULL_MAX_GROUPS, fx.HULL_MAX_CHAINS, fx.HULL_LDS_POINTS, fx.HULL_LABELS_PER_TRIP) == (4096, 32768, 2048, 16384)
    assert (constexpr_int(spatial, "RIPLEY_MAX_R"), constexpr_int(spatial, "RIPLEY_MAX_SIMS")) == (ss.MAX_RADIUS, ss.MAX_SIMS)
    # the caps that are literals of the launch lines
    kernels_h = (CSRC / "kernels.h").read_text()
    assert "inline int grid_for(long work_items, int per_block, long cap = 8192)" in kernels_h and fx.WAVE_UNITS_PER_TRIP == 8192 * 4
    for line in ("grid_for((long)HULL_QUANTITIES * max_out, 256, 1024)", "grid_for(p.slots, 256, 1024)", "grid_for((long)h * ((w + 63) / 64), 4)",
                 "grid_for(2L * max_out, 1, HULL_MAX_CHAINS)", "grid_for(max_out, 4, HULL_MAX_GROUPS)"):
        assert line in hull, line
    assert fx.HULL_WORDS_PER_TRIP == 256 * 1024
    for line in ("grid_for(max_points, 4, std::max(1, 4096 / sets))", "grid_for((long)sets * max_points, 256, 4096)",
                 "for (int base = 0; base < n; base += 256)"):
        assert line in spatial, line
    assert (fx.RIPLEY_PAIR_GROUPS, fx.RIPLEY_SET_POINTS_PER_TRIP, fx.RIPLEY_TABLE_CHUNK) == (4096, 256 * 4096, 256)
    assert "const dim3 flat(grid_for(hw, 256, 4096), n);" in border and fx.BORDER_PIXELS_PER_TRIP == 256 * 4096
    outlines = (CSRC / "outlines.hip").read_text()
    assert constexpr_int(outlines, "OL_THREADS") * constexpr_int(outlines, "OL_ITEMS") == fx.OUTLINE_TILE == 1024
    assert "OL_TILE = OL_THREADS * OL_ITEMS;" in outlines and constexpr_int(outlines, "OL_THREADS") == 256
    assert constexpr_int(outlines, "OL_MAX_GRID") * 256 == fx.OUTLINE_CRACKS_PER_TRIP == 1 << 20
    for line in ("const int crack_grid = grid_for(max_cracks, OL_THREADS, OL_MAX_GRID);", "grid_for(p.corners, OL_THREADS, 8192)",
                 "grid_for((long)OUTLINE_QUANTITIES * max_out, 256, 1024)), dim3(256)",
                 "hipLaunchKernelGGL(ol_scan_cracks_kernel, dim3(1), dim3(1024)", "hipLaunchKernelGGL(ol_scan_contours_kernel, dim3(1), dim3(1024)",
                 "const dim3 block(OL_THREADS);"):
        assert line in outlines, line
    # the scan loop of the two one-workgroup kernels is scan_plane's: a trip is its THREADS, 1024 unless a caller says otherwise
    wave_ops = (CSRC / "wave_ops.h").read_text()
    for line in ("template <int THREADS = 1024>\n__device__ __forceinline__ long long scan_plane(",
                 "for (int base = 0; base < n; base += THREADS)"):
        assert line in wave_ops, line
    assert outlines.count("scan_plane(p.tile_") == 3 and "scan_plane<" not in outlines
    for kernel in ("ol_leader_kernel", "ol_cut_kernel", "ol_rank_kernel"):                      # the loops of one trip of 4096 x 256
        assert f"hipLaunchKernelGGL({kernel}, dim3(crack_grid), block" in outlines, kernel
    assert "hipLaunchKernelGGL(ol_vertices_kernel, dim3(crack_grid), block" in outlines
    assert (fx.OUTLINE_SCAN_TILES_PER_TRIP, fx.OUTLINE_CORNERS_PER_TRIP, fx.OUTLINE_INIT_WORDS_PER_TRIP) == (1024, 8192 * 256, 1024 * 256)
    assert constexpr_int("constexpr int A = 3, B = (1 << 4) / 2 + 1;", "B") == 9                 # the reader itself


def test_run_edge_labels_hold_what_they_are_for():
    lab = fx.run_edge_labels()
    K, big = fx.RUN_EDGE_MAX_OUT, fx.RUN_EDGE_SKIPPED
    assert lab.shape == (6, 130) and lab.dtype == np.int32 and 130 == 2 * 64 + 2
    heads = np.ones_like(lab, bool)                             # lane 0 of a chunk, or a label other than the one before
    heads[:, 1:] = lab[:, 1:] != lab[:, :-1]
    heads[:, [0, 64, 128]] = True
    per_chunk = [[int(heads[y, c:c + 64].sum()) for c in (0, 64, 128)] for y in range(6)]
    assert (lab[0] == 1).all() and per_chunk[0] == [1, 1, 1]                            # runs of 64, 64 and 2
    assert per_chunk[1] == [64, 64, 2] and lab[1].min() >= 1 and lab[1].max() <= K      # every lane a head
    changes = np.flatnonzero(lab[2, 1:] != lab[2, :-1]) + 1
    assert changes.tolist() == [64, 128, 129] and (lab == lab[2, 129]).sum() == 1       # 63|64, 127|128, and a label at 129 only
    assert np.flatnonzero(lab[3]).tolist() == [0, 63, 64] and lab[3, 63] == lab[3, 64] != lab[3, 0]
    at = np.flatnonzero(lab[4] == big)
    assert big > K and at.tolist() == [70] and lab[4, 69] == lab[4, 71] and 1 <= lab[4, 69] <= K
    assert lab[4, 63] == lab[4, 64] == lab[4, 69]                                       # ... a run that also crosses a chunk seam
    assert not lab[5].any()
    assert sorted(set(lab.ravel().tolist()) - {0, big}) == list(range(1, K + 1))
    moved = fx.moved_one_pixel(lab)
    assert np.array_equal(moved[:, 1:], lab[:, :-1]) and not moved[:, 0].any()
    col = fx.moved_one_pixel(lab[:, :1])
    assert col.shape == (6, 1) and np.array_equal(col[1:], lab[:-1, :1]) and col[0, 0] == 0


def test_hull_sparse_fixture_reaches_four_trips():
    compact, high, numbers = cf.hull_sparse_maps()
    max_out = cf.HULL_SPARSE_MAX_OUT
    assert max_out == 65536 and high.shape == (96, 130) and len(numbers) == len(set(numbers.tolist())) == 14
    cf.assert_hull_sparse_premise(high, max_out)
    with pytest.raises(AssertionError):                      # at one trip's worth of labels the premise does not hold
        cf.assert_hull_sparse_premise(np.where(high <= 16384, high, 0), 16384)
    with pytest.raises(AssertionError):
        cf.assert_hull_sparse_premise(compact, max_out)
    # the expected rows: the compact map's by the plain loops, scattered; the host path on the high numbers gives the same
    ref = hull_ref.label_hull_ref(compact, len(numbers))
    want = cf.scatter_rows(ref, numbers, max_out)
    host = dh.label_hull_numpy(high, max_out)
    assert all(np.array_equal(want[j], host[q]) for j, q in enumerate(dh.QUANTITIES))
    assert np.count_nonzero(want[4]) == 14 and want[4].max() >= 8
    assert cf.rows_needed(high, max_out) == sum(rows for _, _, rows, _ in cf.HULL_SPARSE_SPEC)


def test_hull_columns_fixture_uses_more_slots_than_one_trip():
    lab = cf.hull_columns_map()
    cf.assert_hull_columns_premise(lab)
    assert cf.slots_used(lab, cf.HULL_COLUMNS) == 268928 and lab.shape == (2100, 130)
    with pytest.raises(AssertionError):
        cf.assert_hull_columns_premise(lab[:2000])
    host = dh.label_hull_numpy(lab, cf.HULL_COLUMNS)
    assert all(tuple(int(host[q][k]) for q in dh.QUANTITIES) == cf.rect_integers(2100, 1) for k in range(cf.HULL_COLUMNS))
    assert cf.rect_integers(7, 3) == known_shapes()["rectangle"][2]


def test_hull_limit_fixtures_reach_the_last_column_and_row():
    for name, (lab, hand) in cf.hull_limit_maps().items():
        h, w = lab.shape
        host = dh.label_hull_numpy(lab, 2)
        for k, ints in hand.items():
            assert tuple(int(host[q][k - 1]) for q in dh.QUANTITIES) == ints, (name, k)
        pts = hull_ref.hull_corner_points(lab, 1)
        assert max(p[0] for p in pts) == w if name == "wide" else max(p[1] for p in pts) == h == 16384
    assert dh.label_hull_numpy(cf.hull_limit_maps()["tall"][0], 2)["nv"].tolist() == [4, 6]
    lab = cf.hull_tall_parabolas()
    c, kept = cf.chunk_chain_points(cf.left_candidates(lab, 1), 1)
    assert (c, kept) == (257, 2160) and kept > fx.HULL_LDS_POINTS and cf.rows_needed(lab, 1) == 16384
    small = np.zeros((9, 12), np.int32)
    small[[0, 1, 2, 8], [4, 1, 0, 9]] = 1
    assert cf.left_candidates(small, 1) == [4, 1, 0, 0, None, None, None, None, 9, 9]
    assert cf.label_heights(small, 1) == {1: (0, 9)} and cf.slots_used(small, 1) == 10


def test_ripley_fixtures_reach_the_tiles_trips_and_chunks():
    assert cf.RIPLEY_TILE_COUNTS == (2049, 4100)
    for N in cf.RIPLEY_TILE_COUNTS:
        for windowed in (False, True):
            py, px, win = cf.ripley_tile_points(N, windowed)
            cf.assert_ripley_tiles_premise(N, py, px)
            assert (win is None) != windowed and (win is None or win[py, px].all())
    with pytest.raises(AssertionError):                      # one full tile is not enough
        py, px, _ = cf.ripley_tile_points(2049, False)
        cf.assert_ripley_tiles_premise(2048, py[:2048], px[:2048])
    assert cf.assert_second_i_trip(165, 99) == (40, 2) and cf.assert_second_i_trip(70, 999) == (4, 5)
    for N, S in ((160, 99), (65, 99), (1025, 3)):            # what tests/test_gpu_spatial.py runs: one trip
        with pytest.raises(AssertionError):
            cf.assert_second_i_trip(N, S)
    assert cf.pair_grid(1025, 3) == 257 and cf.pair_grid(65, 99) == 17 and cf.pair_grid(16384, 3) == 1024
    c = cf.RIPLEY_SETS_CASE
    cf.assert_ripley_sets_premise(c["S"], c["N"])
    for S, N in ((999, 1048), (998, 1049)):
        with pytest.raises(AssertionError):
            cf.assert_ripley_sets_premise(S, N)
    for k, cap in ((257, 257), (600, 600), (600, 300), (600, cf.RIPLEY_CAPACITY)):
        area, sy, sx, window = cf.long_table(k)
        assert len(area) == k
        cf.assert_table_chunks_premise(area, sy, sx, 96, 130, window, cap)
    with pytest.raises(AssertionError):
        cf.assert_table_chunks_premise(*cf.long_table(257)[:3], 96, 130, cf.long_table(257)[3], 256)
    for h, w in ((16384, 2), (2, 16384)):
        py, px = cf.ripley_limit_points(h, w)
        assert len(set(zip(py, px))) == len(py) == 10 and max(py) == h - 1 and max(px) == w - 1


def test_ripley_plain_loops_on_the_small_cap_fixtures():
    """The host path that the device is compared with, against the plain loops of tests/spatial_ref.py, where those are quick."""
    h, w = 96, 130
    win = cf.ripley_holes_window(h, w)
    py, px = ss.simulated_points(50 + 165, 0, 165, h, w, win)
    got = ss.ripley_counts_numpy(py, px, h, w, 16, 2, 4321, win)
    want = spatial_ref.ripley_counts(list(zip(py.tolist(), px.tolist())), h, w, 16, 2, 4321, win)
    assert all(np.array_equal(g, np.array(v)) for g, v in zip(got, want))
    area, sy, sx, window = cf.long_table(600)
    pts, dropped = spatial_ref.points_of_table(area.tolist(), sy.tolist(), sx.tolist(), h, w, window)[:2]
    qy, qx, info = ss.droplet_points(area, sy, sx, h, w, window)
    assert [tuple(p) for p in pts] == list(zip(qy.tolist(), qx.tolist())) and info["n_dropped"] == 600 - len(pts)


def test_border_fixture_crosses_the_second_trip():
    masks = cf.border_masks()
    assert masks.shape == (2, 1100, 960) and cf.assert_border_premise(masks) == 1056000 > fx.BORDER_PIXELS_PER_TRIP
    assert divmod(fx.BORDER_PIXELS_PER_TRIP, 960) == (1092, 256)
    with pytest.raises(AssertionError):                      # an image of at most 1 048 576 pixels has no second trip
        cf.assert_border_premise(cf.border_masks((1092, 960)))
    with pytest.raises(AssertionError):
        cf.assert_border_premise(np.stack([masks[0], masks[0]]))


# ---- outlines.hip ----------------------------------------------------------------------------------------------------------------

def test_outline_serpentine_is_one_contour_longer_than_a_trip():
    lab, ref = cf.outline_ref("serpentine")
    assert lab.shape == (1100, 960)
    assert cf.assert_outline_serpentine_premise(lab, ref) == (1058061, 1034, 1057102, 1, 2202, 21)
    from tests.test_gpu_outlines import serpentine
    assert np.array_equal(cf.outline_long_serpentine((96, 130)), serpentine())                # the same rule
    small = cf.outline_long_serpentine((96, 130))            # what tests/test_gpu_outlines.py reaches: one trip, 14 rounds
    rec = do.outlines_numpy(small, 1)
    assert cf.outline_counts(small, rec) == (12707, 12578, 1, 194, 12578) and cf.outline_rounds(12578) == 14
    with pytest.raises(AssertionError):
        cf.assert_outline_serpentine_premise(small, rec)
    assert [cf.outline_rounds(v) for v in (0, 1, 2, 3, 1 << 20, (1 << 20) + 1, 1 << 30, (1 << 30) + 1, 2 ** 31 - 1)] == [0, 0, 1, 2, 20, 21, 30, 31, 31]


def test_outline_checkerboard_has_more_contours_than_a_trip():
    lab, ref = cf.outline_ref("checkerboard")
    assert lab.shape == (728, 728)
    assert cf.assert_outline_checkerboard_premise(lab, ref)[:5] == (531441, 1059968, 264992, 1059968, 1036)
    assert (ref["contours"]["length"] == 4).all() and sorted(np.unique(lab).tolist()) == [0, 1, 2, 3]
    small = cf.outline_checkerboard(96)
    with pytest.raises(AssertionError):
        cf.assert_outline_checkerboard_premise(small, do.outlines_numpy(small, 3))


@pytest.mark.parametrize("shape,counts", zip(fx.CAP_SHAPES, ((2115858, 2067, 338, 59248, 344, 6, 4, 1), (2116722, 2068, 315, 58496, 316, 1, 34, 31))),
                         ids=[f"{s[0]}x{s[1]}" for s in fx.CAP_SHAPES])
def test_cap_label_maps_pass_the_corner_grid_of_the_outlines(shape, counts):
    lab, ref = cf.outline_ref("{}x{}".format(*shape))
    assert lab is fx.cap_labels(shape)[0]
    assert cf.assert_outline_corner_grid_premise(lab, ref) == counts
    h = fx.OUTLINE_CORNERS_PER_TRIP // (shape[1] + 1)        # cut where the second trip would start: no corner past it
    cut = lab[:h - 1]
    with pytest.raises(AssertionError):
        cf.assert_outline_corner_grid_premise(cut, do.outlines_numpy(cut, int(lab.max())))


def test_outline_limit_fixtures_reach_the_last_lattice_lines():
    maps = cf.outline_limit_maps()
    assert sorted(maps) == ["tall", "wide"]
    for name, (lab, hand) in maps.items():
        cf.assert_outline_limit_premise(name, lab, cf.outline_ref(name)[1], hand)
        assert hand[1] == (32770, 1, 0, 4, 32768, 32768)
    with pytest.raises(AssertionError):
        lab = maps["tall"][0][:16383]
        cf.assert_outline_limit_premise("tall", lab, do.outlines_numpy(lab, 2), maps["tall"][1])


def test_outline_blob_map_asks_for_more_room_than_a_trip():
    from unet_dc_segmentation_amd.outlines import rooms_for
    lab = cf.outline_blob_labels()
    area = np.bincount(lab.ravel())[1:]
    rooms = rooms_for(area, connected=False)
    assert lab.shape == (1040, 1388) and rooms["max_cracks"] == rooms["max_len"] == 4 * int((lab > 0).sum()) == 1154852
    assert rooms["max_cracks"] > fx.OUTLINE_CRACKS_PER_TRIP and cf.outline_rounds(rooms["max_len"]) == 21
    assert cf.tiles(1041 * 1389) > fx.OUTLINE_SCAN_TILES_PER_TRIP                              # the crack scan's second trip
    for shape, cracks in zip(fx.CAP_SHAPES, (1685856, 1690116)):                                # what the flow asks for on the cap maps
        a = np.bincount(fx.cap_labels(shape)[0].ravel())[1:]
        assert rooms_for(a, connected=False)["max_cracks"] == cracks and cf.tiles(cracks) > fx.OUTLINE_SCAN_TILES_PER_TRIP
    assert fx.OUTLINE_INIT_WORDS_PER_TRIP < 6 * 65536 and 6 * 43690 <= fx.OUTLINE_INIT_WORDS_PER_TRIP < 6 * 43691


def test_workspace_queries_cover_the_planes_the_launchers_lay_out(lib):
    """unetdc_split_stats keeps the planes of unetdc_ccl_stats (64-byte aligned), then D2, then B; B is the workspace it hands
    the distance transform, whose documented need is 4 h w + 64 bytes.  unetdc_ccl_labels keeps the ccl planes and one int32
    plane.  A query that names less than that lets the last plane run past the workspace."""
    for h, w in ((1, 1), (5, 64), (37, 53), (96, 130), (276, 408), (300, 401), (3, 4097), (2, 16384), (1040, 1388)):
        n = h * w
        ccl = (lib.unetdc_ccl_workspace(h, w) + 63) // 64 * 64
        assert lib.unetdc_ccl_workspace(h, w) >= 24 * n + 4 * ((n + 1023) // 1024)
        assert lib.unetdc_split_workspace(h, w) >= ccl + 4 * n + (4 * n + 64)
        assert lib.unetdc_ccl_labels_workspace(h, w) >= ccl + 4 * n
        assert lib.unetdc_mask_clean_workspace(h, w) == 8 * n + 64               # as include/unetdc_hip.h states it
        assert lib.unetdc_density_workspace(h, w) >= 20 * n + 8 * 256 + 20 * h + 1040 if min(h, w) >= 2 else lib.unetdc_density_workspace(h, w) == 0
        assert lib.unetdc_label_overlap_workspace(h, w, n) >= 64 + 12 * 2 * n + 12 * n
