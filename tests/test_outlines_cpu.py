"""CPU: droplet outlines as polygons.  utils/droplet_outlines.py against the known answers of the
definition and against invariants that do not share its code (SciPy's labelling, an even-odd refill at pixel centres); the ring
grouping and the two writers; outline_columns; the script's flag on the CPU path; the host-only checks of
unetdc_label_outlines."""
import ctypes
import json

import numpy as np
import pandas as pd
import pytest
from scipy import ndimage

from tests.test_confidence_cpu import BASE_COLUMNS, files, run_script
from utils import droplet_outlines as do

Q = do.QUANTITIES


def minus(h, w, *holes):
    m = np.ones((h, w), np.int32)
    for r, c in holes:
        m[r, c] = 0
    return m


def known_shapes():
    """name -> (label map, {label: [(start id, L, S2, nv), ...]}, {(label, contour): vertices}): the table of DESIGN.md
    section 27."""
    plus = np.zeros((3, 3), np.int32)
    plus[1, :] = plus[:, 1] = 1
    ring = minus(5, 5, *[(r, c) for r in (1, 2, 3) for c in (1, 2, 3)])
    ring[2, 2] = 2
    yy, xx = np.mgrid[-40:41, -40:41]
    return {
        "pixel": (np.ones((1, 1), np.int32), {1: [(0, 4, 2, 4)]}, {(1, 0): [(0, 0), (1, 0), (1, 1), (0, 1)]}),
        "rectangle": (np.ones((3, 7), np.int32), {1: [(0, 20, 42, 4)]}, {}),
        "plus": (plus, {1: [(4, 12, 10, 12)]}, {}),
        "diagonal": (np.eye(5, dtype=np.int32), {1: [(28 * i, 4, 2, 4) for i in range(5)]}, {}),
        "square minus centre": (minus(3, 3, (1, 1)), {1: [(0, 12, 18, 4), (21, 4, -2, 4)]}, {(1, 1): [(1, 1), (1, 2), (2, 2), (2, 1)]}),
        "diagonal hole": (minus(5, 5, (1, 1), (2, 2), (3, 3)), {1: [(0, 20, 50, 4), (29, 12, -6, 12)]}, {}),
        "two holes": (minus(4, 5, (1, 1), (2, 3)), {1: [(0, 18, 40, 4), (29, 4, -2, 4), (61, 4, -2, 4)]}, {}),
        "ring with a core": (ring, {1: [(0, 20, 50, 4), (29, 12, -18, 4)], 2: [(56, 4, 2, 4)]}, {}),
        "disc": ((yy * yy + xx * xx <= 1600).astype(np.int32), {1: [(40 * 4, 324, 10050, 196)]}, {}),
    }


KNOWN_ROWS = {"diagonal": (20, 5, 0, 20, 10, 10), "square minus centre": (16, 1, 1, 8, 18, 16)}


def known_map():
    """The known-answer shapes but the disc in one 16 x 48 label map, one pair of labels each (the core of the ring keeps its
    own), a background column between neighbours except where the rectangle touches the plus."""
    lab = np.zeros((16, 48), np.int32)
    y, x, k = 1, 1, 0
    for name, (m, _, _) in known_shapes().items():
        if name == "disc":
            continue
        h, w = m.shape
        if x + w > lab.shape[1]:
            y, x = y + 7, 1
        lab[y:y + h, x:x + w][m > 0] = (m + k)[m > 0]
        k += int(m.max())
        x += w + (0 if name == "rectangle" else 1)
    return lab


def random_labels(h, w, seed, top=3):
    return np.random.default_rng(seed).integers(0, top + 1, size=(h, w)).astype(np.int32)


def fill_mask(h, w, seed, fill=0.6):
    return (np.random.default_rng(seed).random((h, w)) < fill).astype(np.int32)


def contours_of(rec, k, w):
    """[(start id, L, S2, nv), ...] of label k, the start id from the first vertex and the direction to the second."""
    c, out = rec["contours"], []
    for i in np.flatnonzero(c["label"] == k):
        a = int(c["first"][i])
        x0, y0, x1, y1 = (int(v) for v in (rec["x"][a], rec["y"][a], rec["x"][a + 1], rec["y"][a + 1]))
        d = 0 if x1 > x0 else 2 if x1 < x0 else 1 if y1 > y0 else 3
        out.append(((y0 * (w + 1) + x0) * 4 + d, int(c["length"][i]), int(c["S2"][i]), int(c["nv"][i])))
    return out


def refill(rec, k, h, w):
    """label == k from the contours of k alone: the even-odd rule at every pixel centre, by toggling everything left of each
    vertical edge."""
    acc = np.zeros((h, w), np.int64)
    for i in np.flatnonzero(rec["contours"]["label"] == k):
        pts = do.ring(rec, i, closed=True)
        for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
            if x0 == x1:
                acc[min(y0, y1):max(y0, y1), :x0] += 1
    return acc % 2 == 1


def check_invariants(lab, n):
    rec = do.outlines_numpy(lab, n)
    h, w = lab.shape
    c = rec["contours"]
    assert len(rec["x"]) == len(rec["y"]) == int(c["nv"].sum()) and rec["x"].dtype == rec["y"].dtype == np.int32
    assert np.array_equal(c["first"], np.cumsum(c["nv"]) - c["nv"]) and (c["nv"] >= 4).all() and (c["S2"] != 0).all()
    starts = {i: s for k in range(1, n + 1) for i, (s, *_) in zip(np.flatnonzero(c["label"] == k), contours_of(rec, k, w))}
    assert all(starts[i] < starts[i + 1] for i in range(len(c["label"]) - 1))          # listed in ascending start id
    for i in range(len(c["label"])):                         # no three consecutive vertices on a line; unit steps add up
        p = np.array(do.ring(rec, i), np.int64)
        e = np.roll(p, -1, axis=0) - p
        assert ((e[:, 0] == 0) != (e[:, 1] == 0)).all() and int(np.abs(e).sum()) == c["length"][i]
        f = np.roll(e, -1, axis=0)
        assert (e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0] != 0).all(), i
        assert int(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])) == c["S2"][i]
    for k in range(1, n + 1):
        m = lab == k
        r = {q: int(rec["rows"][q][k - 1]) for q in Q}
        if not m.any():
            assert not any(r.values())
            continue
        assert r["S2"] == 2 * int(m.sum())
        assert r["no"] == ndimage.label(m)[1]
        comp, ncomp = ndimage.label(np.pad(~m, 1, constant_values=True), structure=np.ones((3, 3)))
        assert r["nh"] == ncomp - 1
        mine = c["label"] == k
        assert r["E"] == c["length"][mine].sum() and r["nv"] == c["nv"][mine].sum() and r["F2"] == c["S2"][mine & (c["S2"] > 0)].sum()
        assert np.array_equal(refill(rec, k, h, w), m)
    assert not np.isin(c["label"], [0] + list(range(n + 1, int(lab.max(initial=0)) + 1))).any()
    return rec


# ---- the rule --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(known_shapes()))
def test_known_answers(name):
    lab, want, verts = known_shapes()[name]
    rec = check_invariants(lab, int(lab.max()))
    for k, cs in want.items():
        assert contours_of(rec, k, lab.shape[1]) == cs
    for (k, j), v in verts.items():
        i = np.flatnonzero(rec["contours"]["label"] == k)[j]
        assert [tuple(p) for p in do.ring(rec, i)] == v
    if name in KNOWN_ROWS:
        assert tuple(int(rec["rows"][q][0]) for q in Q) == KNOWN_ROWS[name]
    if name == "disc":
        assert lab.sum() == 5025 and len(rec["contours"]["label"]) == 1


def test_known_map_holds_every_small_shape():
    lab = known_map()
    rec = check_invariants(lab, int(lab.max()))
    assert lab.max() == 9 and sorted(np.unique(lab)) == list(range(10))
    want = [v for name, (_, cs, _) in known_shapes().items() if name != "disc" for k in sorted(cs) for v in [[c[1:] for c in cs[k]]]]
    assert [[c[1:] for c in contours_of(rec, k, 48)] for k in range(1, 10)] == want


def test_invariants_on_random_maps():
    rng = np.random.default_rng(27)
    for t in range(300):
        h, w = (int(v) for v in rng.integers(1, 9, size=2))
        check_invariants(random_labels(h, w, 1000 + t), 3)
    for t in range(20):
        check_invariants(fill_mask(24, 31, 2000 + t), 1)


def test_capacity_skips_labels_and_keeps_them_as_not_k():
    lab = random_labels(9, 11, 5, top=5)
    rec = check_invariants(lab, 3)
    low = do.outlines_numpy(np.where(lab > 3, 0, lab), 3)    # a skipped label is background to the others
    assert all(np.array_equal(rec["rows"][q], low["rows"][q]) for q in Q) and np.array_equal(rec["x"], low["x"])
    zero = do.outlines_numpy(lab, 0)
    assert all(zero["rows"][q].shape == (0,) for q in Q) and len(zero["contours"]["label"]) == 0 and len(zero["x"]) == 0


# ---- rings and the writers ------------------------------------------------------------------------------------------------------

def two_pieces():
    """Label 1: a 5 x 5 ring whose pocket holds a 1-pixel piece of the same label diagonal to nothing, and a second piece, a
    3 x 3 square minus its centre, to the right; label 2: one pixel."""
    lab = np.zeros((7, 12), np.int32)
    lab[1:6, 1:6] = minus(5, 5, *[(r, c) for r in (1, 2, 3) for c in (1, 2, 3)])
    lab[3, 3] = 1
    lab[2:5, 7:10] = minus(3, 3, (1, 1))
    lab[0, 11] = 2
    return lab


def test_rings_assign_holes_to_the_piece_that_owns_them():
    lab = two_pieces()
    rec = check_invariants(lab, 2)
    g = do.rings(rec)
    assert list(g) == [1, 2] and g[2] == [(int(np.flatnonzero(rec["contours"]["label"] == 2)[0]), [])]
    c = rec["contours"]
    by_area = {int(c["S2"][o]): [int(c["S2"][i]) for i in hs] for o, hs in g[1]}
    assert by_area == {50: [-18], 2: [], 18: [-2]}
    # nested pieces: the hole of an inner ring belongs to the inner ring, not to the ring around it
    nest = np.zeros((9, 9), np.int32)
    nest[0, :] = nest[8, :] = nest[:, 0] = nest[:, 8] = 1
    nest[3:6, 3:6] = minus(3, 3, (1, 1))
    rec = check_invariants(nest, 1)
    c = rec["contours"]
    assert {int(c["S2"][o]): [int(c["S2"][i]) for i in hs] for o, hs in do.rings(rec)[1]} == {162: [-98], 18: [-2]}


def geojson_refill(doc, h, w):
    lab = np.zeros((h, w), np.int32)
    for f in doc["features"]:
        g = f["geometry"]
        polys = [g["coordinates"]] if g["type"] == "Polygon" else g["coordinates"]
        acc = np.zeros((h, w), np.int64)
        for poly in polys:
            for pts in poly:
                assert pts[0] == pts[-1] and len(pts) >= 5
                for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
                    if x0 == x1:
                        acc[min(y0, y1):max(y0, y1), :x0] += 1
        assert not lab[acc % 2 == 1].any()
        lab[acc % 2 == 1] = f["properties"]["label"]
    return lab


@pytest.mark.parametrize("lab", [two_pieces(), known_map(), random_labels(8, 8, 3)], ids=["pieces", "known", "random"])
def test_geojson_and_coco(lab):
    n = int(lab.max())
    rec = do.outlines_numpy(lab, n)
    doc = json.loads(json.dumps(do.geojson(rec, "im0", px_per_um=2.0)))
    assert doc["type"] == "FeatureCollection" and doc["name"] == "im0"
    assert np.array_equal(geojson_refill(doc, *lab.shape), lab)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    for f in doc["features"]:
        k = f["properties"]["label"]
        assert f["properties"]["area"] == area[k] and f["properties"]["area_sqmicron"] == area[k] / 4.0
        assert f["geometry"]["type"] == ("MultiPolygon" if rec["rows"]["no"][k - 1] > 1 else "Polygon")
    assert "area_sqmicron" not in do.geojson(rec, "im0")["features"][0]["properties"]
    anns = json.loads(json.dumps(do.coco_annotation(rec, image_id=7, category_id=2, first_id=10)))
    assert [a["id"] for a in anns] == list(range(10, 10 + len(anns))) and {a["image_id"] for a in anns} == {7}
    for a in anns:
        k = a["label"]
        ys, xs = np.nonzero(lab == k)
        assert a["area"] == area[k] and a["holes"] == rec["rows"]["nh"][k - 1] and len(a["segmentation"]) == rec["rows"]["no"][k - 1]
        assert a["bbox"] == [xs.min(), ys.min(), xs.max() + 1 - xs.min(), ys.max() + 1 - ys.min()] and a["category_id"] == 2
        assert all(len(s) >= 8 and len(s) % 2 == 0 for s in a["segmentation"])


def test_columns_on_the_ring_and_the_disc():
    ring = known_shapes()["ring with a core"][0]
    cols = do.outline_columns(do.outlines_numpy(ring, 2), [16, 1], px_per_um=2.0)
    assert list(cols) == list(do.COLUMN_NAMES + do.MICRON_COLUMN_NAMES)
    want = {"perimeter_crack": [32, 4], "n_holes": [1, 0], "euler_number": [0, 1], "area_filled": [25.0, 1.0],
            "hole_area": [9.0, 0.0], "outline_vertices": [8, 4], "perimeter_crack_micron": [16.0, 2.0],
            "area_filled_sqmicron": [6.25, 0.25]}
    for k, v in want.items():
        assert cols[k].tolist() == v, k
    assert cols["area_filled"].dtype == cols["hole_area"].dtype == np.float64
    assert do.outline_summary(cols) == {"n_with_holes": 1, "hole_area_total": 9.0}
    disc = known_shapes()["disc"][0]
    cols = do.outline_columns(do.outlines_numpy(disc, 1), [5025])
    assert list(cols) == list(do.COLUMN_NAMES)
    assert [cols[k].tolist() for k in do.COLUMN_NAMES] == [[324], [0], [1], [5025.0], [0.0], [196]]
    with pytest.raises(ValueError):
        do.outline_columns(do.outlines_numpy(disc, 1), [5024])
    empty = do.outline_columns(do.outlines_numpy(np.zeros((3, 3), np.int32), 0), [])
    assert list(empty) == list(do.COLUMN_NAMES) and all(len(v) == 0 for v in empty.values())


# ---- the script ------------------------------------------------------------------------------------------------------------------

def read_csv(path):
    return pd.read_csv(path, float_precision="round_trip")


def test_script_cpu_path(tmp_path, monkeypatch):
    sizes = ((48, 48), (40, 56))
    with monkeypatch.context() as mp:                        # without the flag the stage's code is never reached
        for fn in ("outlines_numpy", "outline_columns", "geojson", "coco_annotation"):
            mp.setattr(do, fn, None)
        plain = run_script(tmp_path, mp, "plain", [], sizes=sizes)
    base = sorted(["all_droplets.csv", "droplet_size_stats.csv", "summary_per_image.csv"] +
                  [f"im{i}_droplets.csv" for i in range(2)] + [f"predicted_masks/im{i}_pred.png" for i in range(2)])
    assert files(plain) == base
    assert list(read_csv(plain / "all_droplets.csv").columns) == BASE_COLUMNS
    assert list(read_csv(plain / "summary_per_image.csv").columns) == ["filename", "droplet_count", "total_area_px"]
    out = run_script(tmp_path, monkeypatch, "outlines", ["--outlines"], sizes=sizes)
    assert files(out) == sorted(base + ["outlines_coco.json"] + [f"outlines/im{i}.geojson" for i in range(2)])
    for f in base:                                           # the stage reads; nothing the flow computed before moves
        if not f.endswith("droplets.csv") and f != "summary_per_image.csv":
            assert (plain / f).read_bytes() == (out / f).read_bytes(), f
    a, b = read_csv(plain / "all_droplets.csv"), read_csv(out / "all_droplets.csv")
    cols = list(do.COLUMN_NAMES)
    assert list(b.columns) == BASE_COLUMNS + cols and len(b) > 4 and b[BASE_COLUMNS].equals(a)
    assert list(read_csv(out / "im0_droplets.csv").columns) == BASE_COLUMNS + cols
    assert (b["area_filled"] == b["area"] + b["hole_area"]).all() and (b["euler_number"] == 1 - b["n_holes"]).all()
    assert (b["perimeter_crack"] >= 4).all() and (b["outline_vertices"] >= 4).all()
    s = read_csv(out / "summary_per_image.csv")
    assert list(s.columns) == ["filename", "droplet_count", "total_area_px"] + list(do.SUMMARY_NAMES)
    from PIL import Image
    from utils.droplet_match import gt_labels_numpy
    coco = json.loads((out / "outlines_coco.json").read_text())
    assert [im["file_name"] for im in coco["images"]] == ["im0.png", "im1.png"] and len(coco["annotations"]) == len(b)
    assert [(im["height"], im["width"]) for im in coco["images"]] == list(sizes)
    assert [a_["id"] for a_ in coco["annotations"]] == list(range(1, len(b) + 1)) and len(coco["categories"]) == 1
    for i, (h, w) in enumerate(sizes):
        rows = b[b["filename"] == f"im{i}.png"]
        assert s["n_with_holes"][i] == int((rows["n_holes"] > 0).sum()) and s["hole_area_total"][i] == rows["hole_area"].sum()
        mask = (np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0).astype(np.uint8)
        doc = json.loads((out / "outlines" / f"im{i}.geojson").read_text())
        lab = geojson_refill(doc, h, w)                      # the polygons give the droplets back: the components of --min_area 2
        assert np.array_equal(lab, gt_labels_numpy(mask, 2)) and lab.max() == len(rows) == len(doc["features"])
        assert np.array_equal(np.bincount(lab.ravel())[1:], rows["area"].to_numpy())
        assert [a_["area"] for a_ in coco["annotations"] if a_["image_id"] == i + 1] == rows["area"].tolist()
    um = read_csv(run_script(tmp_path, monkeypatch, "um", ["--outlines", "--px_per_micron", "2"], sizes=sizes) / "all_droplets.csv")
    assert set(do.MICRON_COLUMN_NAMES) <= set(um.columns) and np.array_equal(um["perimeter_crack_micron"], b["perimeter_crack"] / 2.0)


def test_script_follows_the_cuts_on_the_cpu_path(tmp_path, monkeypatch):
    """With --split_touching the outlines read the split label map: the polygons refill to the 16-bit label image."""
    from PIL import Image
    sizes = ((48, 48), (40, 56))
    out = run_script(tmp_path, monkeypatch, "combo", ["--outlines", "--split_touching", "--droplet_shape", "--droplet_hull"], sizes=sizes)
    t = read_csv(out / "all_droplets.csv")
    assert set(do.COLUMN_NAMES) <= set(t.columns) and {"perimeter", "solidity"} <= set(t.columns)
    for i, (h, w) in enumerate(sizes):
        lab = np.array(Image.open(out / "predicted_masks" / f"im{i}_labels.png")).astype(np.int32)
        doc = json.loads((out / "outlines" / f"im{i}.geojson").read_text())
        assert np.array_equal(geojson_refill(doc, h, w), lab)
        rows = t[t["filename"] == f"im{i}.png"]
        want = do.outline_columns(do.outlines_numpy(lab, int(lab.max())), np.bincount(lab.ravel())[1:])
        assert all(np.array_equal(rows[k].to_numpy(), want[k]) for k in do.COLUMN_NAMES)


# ---- the C ABI, host only ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_workspace_query_answers_zero_for_what_the_call_refuses(lib):
    q = lib.unetdc_label_outlines_workspace
    sizes = [(1, 1), (1, 64), (37, 53), (96, 130), (1040, 1388), (16384, 16384)]
    for h, w in sizes:
        small = q(h, w, 0, 0)
        assert small > 0 and q(h, w, 7, 0) == small          # the per-label rows live in the output, not in the workspace
        assert q(h, w, 7, 1000) > small and q(h, w, 7, 2000) - q(h, w, 7, 1000) <= 1000 * 64
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (-1, 5, 1, 1), (16385, 5, 1, 1), (5, 16385, 1, 1), (32768, 32768, 1, 1), (5, 5, -1, 1), (5, 5, 1, -1)):
        assert q(*bad) == 0, bad
    assert q(16384, 16384, 1 << 20, 1 << 30) > 52 << 30 and q(16384, 16384, 1 << 20, (1 << 30) + 1) == 0


def test_launcher_refuses_before_any_hip_call(lib):
    """Host memory stands in for device memory: every refusal below comes back before a launch could touch it."""
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    need = lib.unetdc_label_outlines_workspace(5, 7, 8, 100)
    assert 0 < need < (1 << 15)
    ws = a + 4096

    def call(**kw):
        p = dict(label=a, max_out=8, h=5, w=7, max_len=100, ws=ws, nbytes=need, out=a, contours=a, max_contours=25, vx=a, vy=a,
                 max_vertices=100, max_cracks=100, needed=a)
        p.update(kw)
        rc = lib.unetdc_label_outlines(p["label"], p["max_out"], p["h"], p["w"], p["max_len"], p["ws"], p["nbytes"], p["out"], p["contours"],
                                       p["max_contours"], p["vx"], p["vy"], p["max_vertices"], p["max_cracks"], p["needed"], None)
        return rc, lib.unetdc_last_error()

    rc, err = call(nbytes=need - 1)
    assert rc == -3 and err.startswith(b"label_outlines") and b"workspace too small" in err, (rc, err)
    for kw, msg in ((dict(h=0), b"geometry"), (dict(w=16385), b"geometry"), (dict(h=-1), b"geometry"), (dict(max_out=-1), b"geometry"),
                    (dict(max_cracks=-1), b"geometry"), (dict(max_len=-1), b"limit"), (dict(max_contours=-1), b"limit"),
                    (dict(max_vertices=-1), b"limit"), (dict(label=None), b"null"), (dict(ws=None), b"null"), (dict(out=None), b"null"),
                    (dict(contours=None), b"null"), (dict(vx=None), b"null"), (dict(vy=None), b"null"), (dict(needed=None), b"null"),
                    (dict(ws=ws + 1), b"aligned")):
        rc, err = call(**kw)
        assert rc == -1 and err.startswith(b"label_outlines") and msg in err, (kw, rc, err)
    assert bytes(buf.raw) == bytes(1 << 16)
