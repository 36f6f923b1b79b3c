"""GPU: polygons -> label map (csrc/polyfill.hip, unet_dc_segmentation_amd/polygons.py) against the host
restatement utils.polygon_masks.rasterize_numpy, bit for bit.  Every buffer of a direct call sits between canaries
(tests/image_canaries.py), the workspace in one of the states of tests/workspace_states.py, the output plane pre-filled.

The grid cap: pf_fill_kernel runs PF_WAVES = 4 items (polygon, row) per workgroup and trip on at most PF_MAX_GRID = 2048
workgroups, 8192 items per trip.  The 70 000 unit squares are 70 000 items (9 trips, the last one ragged), the one polygon on
16384 x 2 is 16 384 items (2 trips of one polygon); pf_scan_kernel scans 1024 polygons per trip, so the squares are 69 of its trips."""
import json

import numpy as np
import pytest
import torch

from tests import polygon_cases as pc
from tests.image_canaries import Canaried, canaried_like, check_all
from tests.workspace_states import STATES, holds, prepare
from utils import droplet_outlines as do
from utils import polygon_masks as pm

pytestmark = pytest.mark.gpu

ITEMS_PER_TRIP = 4 * 2048
PREFILL = 0x7F
EWORKSPACE = -3


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def stale():
    return torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=1 << 16, dtype=np.uint8)).cuda()


def geometry(packed):
    return len(packed["poly_label"]), len(packed["ring_first"]) - 1, len(packed["verts"])


def device_fill(lib, packed, h, w, state="a5", stale=None, short=0):
    """One unetdc_polygon_fill between canaries -> (return code, the output plane as int32 [h, w], the workspace view)."""
    P, R, V = geometry(packed)
    need = lib.unetdc_polygon_fill_workspace(h, w, P, R, V)
    assert need > 0
    arrays = [canaried_like(np.ascontiguousarray(packed[k], dtype=np.int32)) for k in ("verts", "ring_first", "poly_first_ring", "poly_label")]
    out = Canaried(4 * h * w)
    out.u8.fill_(PREFILL)
    ws = prepare(Canaried(need - short), state, stale)
    rc = lib.unetdc_polygon_fill(arrays[0].ptr if P else None, arrays[1].ptr, arrays[2].ptr, arrays[3].ptr if P else None, P, R, V, h, w,
                                 out.ptr, ws.ptr, ws.nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_all(out, ws, *arrays)
    for a, k in zip(arrays, ("verts", "ring_first", "poly_first_ring", "poly_label")):
        assert np.array_equal(a.numpy(np.int32, -1), np.asarray(packed[k], np.int32).reshape(-1)), k      # inputs are read only
    return rc, out.numpy(np.int32, h, w), ws


def check_fill(lib, features, h, w, state="a5", stale=None):
    packed = pm.pack(features)
    rc, got, _ = device_fill(lib, packed, h, w, state, stale)
    assert rc == 0, lib.unetdc_last_error()
    want = pm.rasterize_numpy(packed, h, w)["labels"]
    assert np.array_equal(got, want)
    return got


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def test_random_polygons_in_every_workspace_state(lib, stale):
    for t, want in enumerate(pc.random_answers()):
        feats, h, w = pc.random_case(t)
        got = check_fill(lib, feats, h, w, STATES[t % len(STATES)], stale)
        assert np.array_equal(got, want), t                  # and the brute force itself


@pytest.mark.parametrize("name", list(pc.known_answers()))
def test_known_answers(lib, name):
    feats, h, w, want = pc.known_answers()[name]
    assert check_fill(lib, feats, h, w).tolist() == want


@pytest.mark.parametrize("w", [1, 63, 64, 65, 128, 129])
def test_word_boundaries(lib, w):
    """The row's bit mask in 64-bit words: a polygon over the full width with a hole across column 64; its left edge toggles at
    k = 0 and its right edge at k = w.  Then the same from outside the image: toggles left of column 0 and right of w."""
    hole = [(63.25, 0.25), (65.25, 0.25), (65.25, 2.75), (63.25, 2.75)]
    got = check_fill(lib, [pc.feature(3, [[(0, 0), (w, 0), (w, 3), (0, 3)], hole])], 3, w)
    want = np.full((3, w), 3, np.int32)
    want[:, 63:65] = 0                                       # the centres 63.5 and 64.5 lie inside the hole
    assert np.array_equal(got, want)
    got = check_fill(lib, [pc.feature(3, [[(-5, -1), (w + 5, -1), (w + 5, 9), (-5, 9)], hole])], 3, w)
    assert np.array_equal(got, want)
    slanted = [pc.feature(2, [[(-0.5, 0), (w - 0.5, 0), (w + 0.5, 3), (0.5, 3)]])]      # crossings on centres at both ends of row 1
    check_fill(lib, slanted, 3, w)


def star(n, cy, cx, r_out, r_in):
    a = np.arange(n) * (2 * np.pi / n)
    r = np.where(np.arange(n) % 2 == 0, r_out, r_in)
    return np.stack((cx + r * np.cos(a), cy + r * np.sin(a)), axis=1)


def test_edge_loop_trips(lib, stale):
    """More edges than the 64 lanes of one trip: a star of 1000 vertices on 40 x 300 (16 trips per row), and a polygon with
    three holes (four rings, the ring loop)."""
    got = check_fill(lib, [pc.feature(7, [star(1000, 20.3, 150.2, 160.0, 11.0)])], 40, 300, "stale", stale)
    assert 500 < np.count_nonzero(got) < 40 * 300
    holes = [[(2.2 + 9 * j, 2.1), (8.7 + 9 * j, 3.3), (6.1 + 9 * j, 9.8)] for j in range(3)]
    got = check_fill(lib, [pc.feature(2, [[(0.3, 0.2), (29.6, 0.4), (28.1, 11.7), (1.2, 11.1)]] + holes)], 12, 31, "ones")
    assert (got[5, [4, 13, 22]] == 0).all() and got[5, 1] == 2


def unit_squares(n, side):
    """n unit squares, square i on pixel (i // side, i % side) with label i + 1, packed without a Python loop."""
    i = np.arange(n)
    x, y = (i % side) * 256, (i // side) * 256
    verts = np.stack((np.stack((x, x + 256, x + 256, x), axis=1), np.stack((y, y, y + 256, y + 256), axis=1)), axis=2).reshape(-1, 2)
    return {"verts": verts.astype(np.int32), "ring_first": (4 * np.arange(n + 1)).astype(np.int32),
            "poly_first_ring": np.arange(n + 1, dtype=np.int32), "poly_label": (i + 1).astype(np.int32)}


def test_past_the_item_grid_cap(lib, stale):
    n, side = 70000, 265
    assert n > 8 * ITEMS_PER_TRIP and n % ITEMS_PER_TRIP and n <= side * side
    packed = unit_squares(n, side)
    few = pm.pack([pc.feature(i + 1, [[(i, 0), (i + 1, 0), (i + 1, 1), (i, 1)]]) for i in range(50)])
    assert all(np.array_equal(few[k], unit_squares(50, side)[k]) for k in few)             # the same record pack makes
    rc, got, _ = device_fill(lib, packed, side, side, "stale", stale)
    want = np.zeros(side * side, np.int32)
    want[:n] = np.arange(1, n + 1)
    assert rc == 0 and np.array_equal(got.ravel(), want)
    rows = 3                                                 # the restatement on the first rows, which hold whole squares only
    head = {**packed, "verts": packed["verts"][:4 * rows * side], "ring_first": packed["ring_first"][:rows * side + 1],
            "poly_first_ring": packed["poly_first_ring"][:rows * side + 1], "poly_label": packed["poly_label"][:rows * side]}
    assert np.array_equal(pm.rasterize_numpy(head, rows, side)["labels"], want.reshape(side, side)[:rows])


def test_one_polygon_of_more_rows_than_a_trip(lib):
    h = 16384
    assert h > ITEMS_PER_TRIP
    got = check_fill(lib, [pc.feature(9, [[(0.2, -3.0), (1.9, 5000.4), (2.6, h + 2.0), (-0.7, 9000.5)]])], h, 2, "zero")
    assert h < np.count_nonzero(got) < 2 * h and got[ITEMS_PER_TRIP:].any()      # rows of the second trip are filled too


# ---- outside, overlap ------------------------------------------------------------------------------------------------------------

def test_outside_the_image(lib):
    partly = [pc.feature(1, [[(-4.3, -2.2), (5.1, 3.3), (-3.5, 12.9)]]), pc.feature(2, [[(6.4, 4.2), (15.5, -3.1), (14.2, 14.8)]]),
              pc.feature(3, [[(3.3, 7.7), (9.1, 15.2), (2.2, 13.4)]])]
    got = check_fill(lib, partly, 10, 12)
    assert set(np.unique(got)) == {0, 1, 2, 3}
    away = [pc.feature(5, [[(-9, -9), (-2, -9), (-2, -2)]]), pc.feature(6, [[(20, 3), (30, 3), (30, 8)]]), pc.feature(7, [[(3, 40), (8, 40), (8, 50)]]),
            pc.feature(8, [[(-1e6, 3), (-5, 3.2), (-5, 7)]])]
    assert not check_fill(lib, away, 10, 12).any()
    rc, got, _ = device_fill(lib, pm.pack([]), 10, 12)       # no polygon at all: the pre-filled plane is cleared
    assert rc == 0 and got.shape == (10, 12) and not got.any()


def test_overlap_takes_the_largest_label_and_one_label_unions(lib):
    big = [(0.5, 0.5), (9.5, 0.5), (9.5, 7.5), (0.5, 7.5)]
    feats = [pc.feature(4, [[(1, 1), (7, 1), (7, 6), (1, 6)]]), pc.feature(9, [[(3, 2), (11, 2), (11, 5), (3, 5)]]), pc.feature(2, [big])]
    got = check_fill(lib, feats, 8, 12)
    assert got[3, 5] == 9 and got[1, 2] == 4 and got[6, 1] == 2 and np.array_equal(got, check_fill(lib, feats[::-1], 8, 12))
    two = check_fill(lib, [pc.feature(2, [[(0, 0), (3, 0), (3, 3), (0, 3)]], [[(1, 1), (5, 1), (5, 5), (1, 5)]])], 6, 7)
    assert two[2, 2] == 2 and np.count_nonzero(two) == 9 + 16 - 4


# ---- ABI edge behaviour ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", STATES)
def test_short_workspace_is_refused_and_nothing_is_written(lib, stale, state):
    feats, h, w = pc.random_case(4)
    rc, got, ws = device_fill(lib, pm.pack(feats), h, w, state, stale, short=1)
    assert rc == EWORKSPACE and b"workspace too small" in lib.unetdc_last_error()
    assert (got.view(np.uint8) == PREFILL).all() and holds(ws, state, stale)


def test_refused_geometries(lib):
    q = lib.unetdc_polygon_fill_workspace
    assert q(5, 7, 0, 0, 0) > 0 and q(5, 7, 2, 2, 6) > q(5, 7, 0, 0, 0)
    for bad in ((0, 7, 1, 1, 3), (5, 16385, 1, 1, 3), (32768, 32768, 1, 1, 3), (5, 7, -1, 1, 3), (5, 7, 2, 1, 6), (5, 7, 1, 2, 5),
                (5, 7, (1 << 22) + 1, 1 << 23, 1 << 25), (5, 7, 1, 1, (1 << 24) + 1), (16384, 2, 1 << 17, 1 << 17, 3 << 17)):
        assert q(*bad) < 0, bad
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for bad in ((0, 7, 1, 1, 3), (5, 7, 1, 2, 5)):
        h, w, P, R, V = bad
        rc = lib.unetdc_polygon_fill(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), P, R, V, h, w, buf.data_ptr(), buf.data_ptr(), 4096, None)
        assert rc == -1 and lib.unetdc_last_error().startswith(b"polygon_fill"), bad
    assert lib.unetdc_polygon_fill(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 1, 3, 5, 7, None, buf.data_ptr(), 4096, None) == -1
    assert lib.unetdc_label_census(buf.data_ptr(), 0, 7, 3, buf.data_ptr(), None) == -1
    assert lib.unetdc_label_relabel(buf.data_ptr(), 5, 7, None, 3, None) == -1
    torch.cuda.synchronize()
    assert not buf.any()


def test_the_same_call_twice_is_bitwise_equal(lib, stale):
    packed = pm.pack([pc.feature(7, [star(1000, 20.3, 150.2, 160.0, 11.0)]), pc.feature(3, [star(40, 11.0, 60.0, 30.0, 5.0)])])
    a = device_fill(lib, packed, 40, 300, "stale", stale)[1]
    b = device_fill(lib, packed, 40, 300, "ones")[1]
    assert np.array_equal(a, b)


# ---- census, relabel, the wrapper ------------------------------------------------------------------------------------------------

def test_census_and_relabel_against_bincount_and_the_host_lookup(lib):
    rng = np.random.default_rng(3)
    s = torch.cuda.current_stream().cuda_stream
    for h, w, top in ((1, 1, 1), (37, 53, 9), (130, 257, 300), (5, 70, 3)):
        lab = rng.integers(-2, top + 3, size=(h, w)).astype(np.int32)
        lab[rng.random((h, w)) < 0.5] = 0
        if h == 130:
            lab[40:90, 20:200] = 7                           # whole waves of one value
        d = canaried_like(lab)
        area = Canaried(8 * top, align=8)
        assert lib.unetdc_label_census(d.ptr, h, w, top, area.ptr, s) == 0
        torch.cuda.synchronize()
        check_all(d, area)
        assert np.array_equal(area.numpy(np.int64, top), np.bincount(lab[(lab >= 1) & (lab <= top)], minlength=top + 1)[1:])
        lut = rng.integers(-5, 2 ** 31 - 1, size=top).astype(np.int32)
        lut[0] = 2 ** 31 - 1
        t = canaried_like(lut)
        assert lib.unetdc_label_relabel(d.ptr, h, w, t.ptr, top, s) == 0
        torch.cuda.synchronize()
        check_all(d, t)
        inside = (lab >= 1) & (lab <= top)
        assert np.array_equal(d.numpy(np.int32, h, w), np.where(inside, lut[np.clip(lab, 1, top) - 1], lab))


def assert_records_equal(got, want):
    assert got["labels"].dtype == torch.int32 and got["labels"].is_cuda
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    for k in ("kept", "area"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k


def test_compaction_and_large_labels():
    from unet_dc_segmentation_amd.polygons import rasterize_batch
    big = [(0, 0), (6, 0), (6, 6), (0, 6)]
    feats = [pc.feature(5, [big]), pc.feature(9, [[(0.1, 0.1), (0.4, 0.1), (0.1, 0.4)]]), pc.feature(12, [[(2, 2), (4, 2), (4, 4), (2, 4)]])]
    rec = rasterize_batch([pm.pack(feats)], [(6, 7)], compact=True)[0]
    assert rec["kept"].tolist() == [5, 12] and sorted(np.unique(rec["labels"].cpu().numpy())) == [0, 1, 2]
    assert_records_equal(rec, pm.rasterize_numpy(pm.pack(feats), 6, 7, compact=True))
    assert_records_equal(rasterize_batch([pm.pack(feats)], [(6, 7)], compact=False)[0], pm.rasterize_numpy(pm.pack(feats), 6, 7))
    top = 2 ** 31 - 1
    large = [pc.feature(top - 1, [big]), pc.feature(top, [[(2, 2), (4, 2), (4, 4), (2, 4)]]), pc.feature(top - 7, [[(1, 1), (5, 1), (5, 3)]])]
    rec = rasterize_batch([pm.pack(large)], [(6, 7)], compact=False)[0]
    assert rec["labels"].max().item() == top and rec["kept"].tolist() == [top - 1, top]
    assert_records_equal(rec, pm.rasterize_numpy(pm.pack(large), 6, 7))


def test_large_labels_through_the_entry_point(lib):
    top = 2 ** 31 - 1
    got = check_fill(lib, [pc.feature(top - 1, [[(0, 0), (6, 0), (6, 6), (0, 6)]]), pc.feature(top, [[(2, 2), (4, 2), (4, 4), (2, 4)]])], 6, 7)
    assert got.max() == top and got[0, 0] == top - 1


def test_rasterize_batch_of_mixed_sizes_equals_single_images_and_waits_once(monkeypatch):
    from unet_dc_segmentation_amd.polygons import rasterize_batch
    cases = [pc.random_case(t) for t in (1, 5)]
    packed = [pm.pack(cases[0][0] + [pc.feature(8, [star(9, 3, 3, 5, 2)])]), pm.pack([]), pm.pack(cases[1][0] + [pc.feature(3, [[(0.1, 0.1), (0.4, 0.1), (0.1, 0.4)]])])]
    hws = [(cases[0][1] + 3, cases[0][2] + 2), (4, 9), (cases[1][1], cases[1][2])]
    for compact in (False, True):
        waits = []
        real = torch.Tensor.cpu
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (waits.append(1), real(t, *a, **k))[1])
            out = rasterize_batch(packed, hws, compact=compact)
        assert len(waits) == 1
        for i, (p, hw) in enumerate(zip(packed, hws)):
            want = pm.rasterize_numpy(p, *hw, compact=compact)
            assert_records_equal(out[i], want)
            assert_records_equal(rasterize_batch([p], [hw], compact=compact)[0], want)
        assert not out[1]["labels"].any() and len(out[1]["kept"]) == 0
    assert rasterize_batch([], []) == []


def test_device_round_trip_outlines_to_polygons_is_the_identity():
    from tests.test_outlines_cpu import fill_mask
    from unet_dc_segmentation_amd.outlines import label_outlines_batch
    from unet_dc_segmentation_amd.polygons import rasterize_batch
    maps = [fill_mask(24, 31, 2000 + t) for t in range(4)] + [pc.round_trip_maps()["known map"], pc.round_trip_maps()["island in its hole"]]
    labs = [torch.from_numpy(m).cuda() for m in maps]
    recs = label_outlines_batch(labs, [np.bincount(m.ravel(), minlength=int(m.max()) + 1)[1:] for m in maps], connected=False)
    packed = [pm.pack(pm.features_of_geojson(json.loads(json.dumps(do.geojson(r, "m"))))) for r in recs]
    for m, out in zip(maps, rasterize_batch(packed, [m.shape for m in maps], compact=False)):
        assert np.array_equal(out["labels"].cpu().numpy(), m)


# ---- the scripts -----------------------------------------------------------------------------------------------------------------

def test_script_reads_back_its_own_outlines(tmp_path, monkeypatch, capsys):
    import pandas as pd
    from tests.test_confidence_cpu import files, run_script
    from tests.test_polygons_cpu import SIZES, polygon_arms
    first = run_script(tmp_path, monkeypatch, "first", ["--outlines"], device="cuda", sizes=SIZES)
    back = run_script(tmp_path, monkeypatch, "back", ["--gt_polygons", str(first / "outlines")], device="cuda", sizes=SIZES)
    assert "--gt_polygons: 0 of" in capsys.readouterr().out
    t = pd.read_csv(back / "all_droplets.csv")
    assert len(t) > 4 and (t["gt_iou"] == 1.0).all() and (t["gt_label"] == t["label"]).all()
    m = pd.read_csv(back / "match_per_image.csv")
    assert (m["n_pred"] == m["n_gt"]).all() and (m["tp_95"] == m["n_pred"]).all() and m["n_pred"].iloc[-1] == len(t)
    assert not m[["n_missed", "n_spurious", "n_merged", "n_split"]].to_numpy().any()
    src, poly, png = polygon_arms(tmp_path, monkeypatch, device="cuda")
    assert files(poly) == files(png)
    for f in files(poly):
        assert (poly / f).read_bytes() == (png / f).read_bytes(), f


def test_training_caches_take_their_masks_from_polygons(tmp_path):
    from PIL import Image
    from tests.test_confidence_cpu import disc_images
    from unet_dc_segmentation_amd.device_data import DeviceImageCache, DeviceNativeCache
    from utils.droplet_match import gt_labels_numpy
    sizes, names = ((48, 56), (40, 72)), ["a.png", "b.png"]
    ind, md = tmp_path / "images", tmp_path / "masks"
    ind.mkdir(), md.mkdir()
    polygons = {}
    for name, img in zip(names, disc_images(sizes, seed=3)):
        Image.fromarray(img).save(ind / name)
        feats = pm.features_of_geojson(do.geojson(do.outlines_numpy(gt_labels_numpy(img[..., 0] > 125)), name))
        feats.append(pc.feature(len(feats) + 1, [star(11, 20.4, 30.3, 14.0, 6.5)]))       # and one that is not on the lattice
        polygons[name] = pm.pack(feats)
        filled = pm.rasterize_numpy(polygons[name], *img.shape[:2])["labels"] > 0
        assert 0 < filled.sum() < filled.size
        Image.fromarray(filled.astype(np.uint8) * 255).save(md / name)
    for make in (lambda **kw: DeviceImageCache(str(ind), kw.pop("mask_dir"), names, 64, 15, "cuda", **kw),
                 lambda **kw: DeviceNativeCache(str(ind), kw.pop("mask_dir"), names, 15, "cuda", keep_foreground=True, **kw)):
        files_cache, poly_cache = make(mask_dir=str(md)), make(mask_dir=None, mask_polygons=polygons)
        assert poly_cache.masks.dtype == torch.uint8 and torch.equal(poly_cache.masks, files_cache.masks) and poly_cache.masks.any()
        assert torch.equal(poly_cache.images, files_cache.images)
        if hasattr(files_cache, "foreground"):
            assert all(np.array_equal(a, b) for a, b in zip(poly_cache.foreground, files_cache.foreground))
    with pytest.raises(ValueError, match="no polygons for b.png"):
        DeviceImageCache(str(ind), None, names, 64, 15, "cuda", mask_polygons={"a.png": polygons["a.png"]})
