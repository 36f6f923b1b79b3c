"""CPU: what the inputs and host-side rules of the workspace-state, grid-cap and C-ABI density tests are for
(tests/workspace_states.py, tests/droplet_edge_fixtures.py), checked without a device."""
import numpy as np
import pytest
import torch

from tests import droplet_edge_fixtures as fx
from tests import workspace_states as wss
from tests.image_canaries import CANARY, Canaried
from tests.match_ref import overlap_table_ref
from tests.test_density_cpu import cell_image
from tests.test_match_cpu import kmax
from utils import density as hd
from utils import droplet_match as dm
from utils import droplet_shape as sh


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
