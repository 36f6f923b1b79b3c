"""CPU: convex hull, solidity and Feret integers per droplet.  utils/droplet_hull.py, the script's CPU
path, against the plain-loop restatement tests/hull_ref.py and the known answers of the definition; hull_columns; the host-only
checks of unetdc_label_hull; the script's flag."""
import ctypes
import math

import numpy as np
import pandas as pd
import pytest

from tests import hull_ref
from tests.test_confidence_cpu import BASE_COLUMNS, files, run_script
from utils import droplet_hull as dh

Q = dh.QUANTITIES


def known_shapes():
    """name -> (mask, area, (H2, F2, Wc, Wl, nv)): the table of DESIGN.md section 24, computed by brute force over all pixel
    corners when the definition was written."""
    plus = np.zeros((3, 3), np.int32)
    plus[1, :] = plus[:, 1] = 1
    ell = np.zeros((5, 5), np.int32)
    ell[:, 0] = ell[4, :] = 1
    cee = np.ones((5, 5), np.int32)
    cee[1:4, 1:5] = 0
    two = np.zeros((1, 9), np.int32)
    two[0, 0] = two[0, 8] = 1
    yy, xx = np.mgrid[-40:41, -40:41]
    return {"pixel": (np.ones((1, 1), np.int32), 1, (2, 2, 1, 1, 4)),
            "rectangle": (np.ones((3, 7), np.int32), 21, (42, 58, 21, 49, 4)),
            "plus": (plus, 5, (14, 10, 4, 2, 8)),
            "diagonal": (np.eye(5, dtype=np.int32), 5, (18, 50, 8, 32, 6)),
            "L": (ell, 9, (34, 50, 24, 32, 5)),
            "C": (cee, 13, (50, 50, 25, 25, 4)),
            "two pixels": (two, 2, (18, 82, 9, 81, 4)),
            "disc": ((yy * yy + xx * xx <= 1600).astype(np.int32), 5025, (10282, 6626, 649, 65, 48))}


def known_map():
    """The known-answer shapes tiled into one label map, one label each, with a background pixel between neighbours except
    where the rectangle touches the plus -> (int32 [h, w], [(H2, F2, Wc, Wl, nv) per label])."""
    shapes = known_shapes()
    lab = np.zeros((96, 130), np.int32)
    want, y, x = [], 1, 1
    for k, (name, (m, _, ints)) in enumerate(shapes.items(), start=1):
        h, w = m.shape
        if x + w > lab.shape[1]:
            y, x = y + 8, 1
        lab[y:y + h, x:x + w][m > 0] = k
        want.append(ints)
        x += w + (0 if name == "rectangle" else 1)
    return lab, want


def as_tuple(rec, k):
    return tuple(int(rec[q][k - 1]) for q in Q)


def random_labels(h, w, seed, n_labels=7, max_label=9):
    """Random blobs that touch, a scattered label with empty rows in between (label 3), labels on all four borders, label 5
    absent, labels 8 and 9 above a max_out of 7."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((h, w), np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(14):
        k = int(rng.integers(1, max_label + 1))
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, min(h, w) // 3))
        lab[((yy - cy) ** 2 * rng.integers(1, 4) + (xx - cx) ** 2 <= r * r)] = k
    lab[rng.random((h, w)) < 0.1] = 0
    lab[::5][:, ::7] = 3                                    # scattered: rows without a pixel of label 3 in between
    lab[0, :w // 2], lab[h - 1, w // 2:], lab[:, 0], lab[:h // 2, w - 1] = 1, 2, 4, 6
    lab[lab == 5] = 0
    return lab


SIZES = [(1, 1), (1, 65), (9, 4), (37, 53), (64, 64), (96, 130)]


@pytest.fixture(scope="module")
def random_cases():
    return [(lab, hull_ref.label_hull_ref(lab, 7)) for lab in (random_labels(h, w, seed=h * 1000 + w) for h, w in SIZES)]


def test_known_answers():
    for name, (m, area, ints) in known_shapes().items():
        assert int(m.sum()) == area, name
        assert as_tuple(hull_ref.label_hull_ref(m, 1), 1) == ints, name
        assert as_tuple(dh.label_hull_numpy(m, 1), 1) == ints, name
        assert as_tuple(dh.label_hull_numpy(m), 1) == ints, name                    # default capacity: the largest label
    lab, want = known_map()
    ref, got = hull_ref.label_hull_ref(lab, len(want)), dh.label_hull_numpy(lab, len(want))
    for k, ints in enumerate(want, start=1):
        assert as_tuple(ref, k) == ints and as_tuple(got, k) == ints, k


def test_host_path_equals_restatement(random_cases):
    for lab, ref in random_cases:
        got = dh.label_hull_numpy(lab, 7)
        for q in Q:
            assert got[q].dtype == np.int64 and got[q].shape == (7,) and np.array_equal(got[q], ref[q]), (lab.shape, q)
        assert as_tuple(got, 5) == (0, 0, 0, 0, 0)                                   # a label without pixels keeps the init values
        present = [k for k in range(1, 8) if (lab == k).any()]
        assert all(got["nv"][k - 1] >= 4 and got["H2"][k - 1] >= 2 for k in present)
        if lab.shape[0] > 30:
            assert (lab > 7).any() and {1, 2, 3, 4, 6} <= set(present)
        # a smaller capacity is a prefix; capacity 0 is empty
        small = dh.label_hull_numpy(lab, 2)
        assert all(np.array_equal(small[q], ref[q][:2]) for q in Q)
        assert all(dh.label_hull_numpy(lab, 0)[q].shape == (0,) for q in Q)


def test_scattered_label_skips_empty_rows():
    lab = np.zeros((12, 9), np.int32)
    lab[1, 4] = lab[5, 1] = lab[5, 7] = lab[10, 3] = 1       # rows 2..4 and 6..9 hold no pixel
    ref = hull_ref.label_hull_ref(lab, 1)
    assert as_tuple(dh.label_hull_numpy(lab, 1), 1) == as_tuple(ref, 1) and ref["nv"][0] == 8


def test_tie_break_takes_the_shortest_edge():
    """A square: four edges of equal width and length.  The plus: its four diagonal edges (Wc, Wl) = (4, 2) tie at a squared
    width of 8 and beat the four axis edges (3, 1) at 9.  The 4 x 4 square without its corner pixels: the axis edges (8, 4) at
    16 beat the diagonal ones (6, 2) at 18.  The L of three pixels, where edges of different length tie: the shorter."""
    sq = np.ones((4, 4), np.int32)
    assert as_tuple(dh.label_hull_numpy(sq, 1), 1) == as_tuple(hull_ref.label_hull_ref(sq, 1), 1) == (32, 32, 16, 16, 4)
    plus = known_shapes()["plus"][0]
    assert as_tuple(dh.label_hull_numpy(plus, 1), 1)[2:4] == (4, 2)
    octa = np.ones((4, 4), np.int32)
    octa[0, 0] = octa[0, 3] = octa[3, 0] = octa[3, 3] = 0
    ref = as_tuple(hull_ref.label_hull_ref(octa, 1), 1)
    assert as_tuple(dh.label_hull_numpy(octa, 1), 1) == ref and ref[2:4] == (8, 4)
    # the L of three pixels: hull (0,0) (2,0) (2,1) (1,2) (0,2); width 2 across the edges of length 2 -- (Wc, Wl) = (4, 4) -- and
    # across those of length 1 -- (2, 1): equal ratios, the smaller Wl wins; the diagonal edge has 9 / 2
    tromino = np.array([[1, 1], [1, 0]], np.int32)
    assert as_tuple(dh.label_hull_numpy(tromino, 1), 1) == as_tuple(hull_ref.label_hull_ref(tromino, 1), 1) == (7, 8, 2, 1, 5)


def test_columns():
    shapes = known_shapes()
    names = ["rectangle", "plus", "disc", "pixel"]
    hull = {q: np.array([shapes[n][2][j] for n in names], np.int64) for j, q in enumerate(Q)}
    area = np.array([shapes[n][1] for n in names], np.int64)
    c = dh.hull_columns(hull, area)
    assert tuple(c) == dh.COLUMN_NAMES and all(v.dtype == (np.int64 if k == "hull_vertices" else bool if k == "low_solidity" else np.float64)
                                               for k, v in c.items())
    assert c["solidity"][0] == 1.0 and c["solidity"][1] == 5 / 7 and c["solidity"][3] == 1.0
    assert c["feret_diameter_max"][2] == math.sqrt(6626) and c["feret_diameter_max"][0] == math.sqrt(58)
    assert c["feret_diameter_min"][0] == 3.0 and c["feret_diameter_min"][1] == math.sqrt(8) and c["feret_diameter_min"][2] == math.sqrt(649 * 649 / 65)
    assert np.array_equal(c["area_convex"], [21.0, 7.0, 5141.0, 1.0]) and np.array_equal(c["hull_vertices"], [4, 8, 48, 4])
    assert np.array_equal(c["feret_ratio"], c["feret_diameter_min"] / c["feret_diameter_max"])
    assert c["low_solidity"].tolist() == [False, True, False, False]                # default 0.9: the plus alone
    assert dh.hull_columns(hull, area, 0.5)["low_solidity"].tolist() == [False] * 4
    assert dh.hull_columns(hull, area, 1.0)["low_solidity"].tolist() == [False, True, True, False]
    m = dh.hull_columns(hull, area, 0.9, px_per_um=2.0)
    assert tuple(m) == dh.COLUMN_NAMES + dh.MICRON_COLUMN_NAMES
    assert np.array_equal(m["feret_max_micron"], c["feret_diameter_max"] / 2.0) and np.array_equal(m["area_convex_sqmicron"], c["area_convex"] / 4.0)
    assert dh.hull_summary(c) == {"solidity_median": float(np.median(c["solidity"])),
                                  "feret_max_median": float(np.median(c["feret_diameter_max"])), "n_low_solidity": 1}
    empty = dh.hull_columns({q: np.zeros(0, np.int64) for q in Q}, np.zeros(0, np.int64))
    assert all(len(v) == 0 for v in empty.values()) and dh.hull_summary(empty)["n_low_solidity"] == 0
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            dh.check_solidity(bad)
    # large integers: the ratio is one correctly rounded division
    big = {"H2": np.array([2 ** 29 - 1]), "F2": np.array([2 ** 29]), "Wc": np.array([2 ** 29 - 3]), "Wl": np.array([2 ** 28 + 1]), "nv": np.array([9])}
    cb = dh.hull_columns(big, np.array([2 ** 27]))
    assert cb["feret_diameter_min"][0] == math.sqrt((2 ** 29 - 3) ** 2 / (2 ** 28 + 1)) and cb["solidity"][0] == 2 ** 28 / (2 ** 29 - 1)


def test_area_against_qhull(random_cases):
    spatial = pytest.importorskip("scipy.spatial")
    checked = 0
    for lab, ref in random_cases:
        for k in range(1, 8):
            if (lab == k).any():
                pts = np.array(hull_ref.hull_corner_points(lab, k), np.float64)
                vol = spatial.ConvexHull(pts).volume               # the area, in two dimensions
                assert abs(ref["H2"][k - 1] / 2 - vol) <= 1e-9 * vol, (lab.shape, k)
                checked += 1
    assert checked >= 20


def test_droplet_options_carry_the_flag():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.droplets import DropletOptions, Droplets
    assert not DropletOptions().hull and Droplets(None, None, None, None).hull is None
    o = DropletOptions(hull=True, labels=True)               # the hull route has a label map
    assert o.hull and o.label_map and not DropletOptions().label_map
    with pytest.raises(_lib.UnetdcError):
        DropletOptions(labels=True)


# ---- the C ABI, host only ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_workspace_query(lib):
    q = lib.unetdc_label_hull_workspace
    for h, w in ((0, 5), (5, 0), (-1, 5), (5, -1), (16385, 5), (5, 16385)):
        assert q(h, w, 33, 33) == 0, (h, w)
    assert q(64, 64, -1, 33) == 0 and q(64, 64, 33, -1) == 0 and q(64, 64, 33, 2 ** 28 + 1) == 0
    sizes = [q(h, w, mo, mr) for h, w in ((1, 1), (37, 53), (1040, 1388), (16384, 16384)) for mo in (0, 1, 33, 2 ** 14) for mr in (0, 1, 1000, 2 ** 28)]
    assert all(s > 0 for s in sizes)
    assert q(37, 53, 33, 1000) < q(37, 53, 33, 2000) and q(37, 53, 33, 1000) < q(37, 53, 66, 1000)
    # the label part of the candidate planes is capped by the pixel count: more labels than pixels add no slots
    assert q(2, 2, 10 ** 6, 8) - q(2, 2, 10 ** 6 - 16, 8) == 16 * 4 * 5


def test_refusals_come_before_any_launch(lib):
    """Host memory stands in for device memory: every call below returns before any HIP call, and nothing is written."""
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    ws, out, rows = a, a + (1 << 15), a + (1 << 15) + 4096
    need = lib.unetdc_label_hull_workspace(37, 53, 8, 100)
    assert 0 < need < (1 << 15)
    rc = lib.unetdc_label_hull(a, 8, 37, 53, ws, need - 1, out, rows, 100, None)
    err = lib.unetdc_last_error()
    assert rc == -3 and err.startswith(b"label_hull") and b"workspace too small" in err, (rc, err)
    for kw, msg in ((dict(h=0), b"geometry"), (dict(w=16385), b"geometry"), (dict(h=-1), b"geometry"), (dict(max_out=-1), b"geometry"),
                    (dict(max_rows=-1), b"geometry"), (dict(label=None), b"null"), (dict(ws=None), b"null"), (dict(out=None), b"null"),
                    (dict(rows=None), b"null"), (dict(ws=ws + 1), b"aligned")):
        p = dict(label=a, max_out=8, h=37, w=53, ws=ws, nbytes=need, out=out, rows=rows, max_rows=100)
        p.update(kw)
        rc = lib.unetdc_label_hull(p["label"], p["max_out"], p["h"], p["w"], p["ws"], p["nbytes"], p["out"], p["rows"], p["max_rows"], None)
        err = lib.unetdc_last_error()
        assert rc == -1 and err.startswith(b"label_hull") and msg in err, (kw, rc, err)
    assert bytes(buf.raw) == bytes(1 << 16)


# ---- the script ------------------------------------------------------------------------------------------------------------------

HULL_COLUMNS = list(dh.COLUMN_NAMES)


def read_csv(path):
    return pd.read_csv(path, float_precision="round_trip")


def test_script_cpu_path(tmp_path, monkeypatch):
    sizes = ((48, 48), (40, 56))
    with monkeypatch.context() as mp:                        # without the flag the stage's code is never reached
        mp.setattr(dh, "label_hull_numpy", None)
        mp.setattr(dh, "hull_columns", None)
        plain = run_script(tmp_path, mp, "plain", [], sizes=sizes)
    again = run_script(tmp_path, monkeypatch, "again", [], sizes=sizes)
    assert files(plain) == files(again) == sorted(["all_droplets.csv", "droplet_size_stats.csv", "summary_per_image.csv"] +
                                                   [f"im{i}_droplets.csv" for i in range(2)] + [f"predicted_masks/im{i}_pred.png" for i in range(2)])
    for f in files(plain):
        assert (plain / f).read_bytes() == (again / f).read_bytes(), f
    assert list(read_csv(plain / "all_droplets.csv").columns) == BASE_COLUMNS
    assert list(read_csv(plain / "summary_per_image.csv").columns) == ["filename", "droplet_count", "total_area_px"]
    out = run_script(tmp_path, monkeypatch, "hull", ["--droplet_hull"], sizes=sizes)
    assert files(out) == files(plain)
    for f in files(plain):                                   # the stage reads; nothing the flow computed before moves
        if not f.endswith("droplets.csv") and f != "summary_per_image.csv":
            assert (plain / f).read_bytes() == (out / f).read_bytes(), f
    a, b = read_csv(plain / "all_droplets.csv"), read_csv(out / "all_droplets.csv")
    assert list(b.columns) == BASE_COLUMNS + HULL_COLUMNS and len(b) > 4 and b[BASE_COLUMNS].equals(a)
    assert list(read_csv(out / "im0_droplets.csv").columns) == BASE_COLUMNS + HULL_COLUMNS
    assert b["solidity"].between(0, 1).all() and (b["feret_diameter_min"] <= b["feret_diameter_max"]).all()
    assert (b["area_convex"] >= b["area"]).all() and (b["hull_vertices"] >= 4).all() and (b["feret_diameter_max"] ** 2 >= 2).all()
    assert np.array_equal(b["low_solidity"], b["solidity"] < 0.9)
    s = read_csv(out / "summary_per_image.csv")
    assert list(s.columns) == ["filename", "droplet_count", "total_area_px"] + list(dh.SUMMARY_NAMES)
    for i in range(2):
        rows = b[b["filename"] == f"im{i}.png"]
        assert s["solidity_median"][i] == rows["solidity"].median() and s["n_low_solidity"][i] == int(rows["low_solidity"].sum())
        assert s["feret_max_median"][i] == rows["feret_diameter_max"].median()
    strict = read_csv(run_script(tmp_path, monkeypatch, "strict", ["--droplet_hull", "1.0", "--px_per_micron", "2"], sizes=sizes) / "all_droplets.csv")
    assert set(dh.MICRON_COLUMN_NAMES) <= set(strict.columns) and np.array_equal(strict["low_solidity"], strict["solidity"] < 1.0)
    assert np.array_equal(strict["solidity"], b["solidity"])
    for bad in (["--droplet_hull", "0"], ["--droplet_hull", "1.5"]):
        with pytest.raises(SystemExit):
            run_script(tmp_path, monkeypatch, "bad", bad, sizes=sizes)


def test_script_combinations_on_the_cpu_path(tmp_path, monkeypatch):
    """The stage reads only the final label map: with the split, shape, neighbours, confidence, tiles and TTA its integers are
    those of label_hull_numpy on the labels the flow wrote."""
    sizes = ((48, 48), (40, 56))
    out = run_script(tmp_path, monkeypatch, "combo", ["--droplet_hull", "--split_touching", "--droplet_shape", "--neighbors", "3",
                                                      "--confidence", "--tta", "2"], sizes=sizes)
    t = read_csv(out / "all_droplets.csv")
    assert set(HULL_COLUMNS) <= set(t.columns) and {"perimeter", "nn_label", "prob_mean", "tta_spread_mean"} <= set(t.columns)
    from PIL import Image
    lab = np.array(Image.open(out / "predicted_masks" / "im1_labels.png")).astype(np.int32)
    rows = t[t["filename"] == "im1.png"]
    want = dh.hull_columns(dh.label_hull_numpy(lab, int(lab.max())), np.bincount(lab.ravel())[1:])
    assert len(rows) == lab.max() > 0 and np.array_equal(rows["solidity"].to_numpy(), want["solidity"])
    assert np.array_equal(rows["feret_diameter_min"].to_numpy(), want["feret_diameter_min"])
    tiled = run_script(tmp_path, monkeypatch, "tiled", ["--droplet_hull", "--tile", "64", "--tile_overlap", "16"], sizes=((96, 130),))
    assert list(read_csv(tiled / "all_droplets.csv").columns) == BASE_COLUMNS + HULL_COLUMNS
