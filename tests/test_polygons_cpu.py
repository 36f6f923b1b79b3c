"""CPU: polygon annotations back into label maps.  utils/polygon_masks.py against a brute-force
point-in-polygon test that shares none of its code (tests/polygon_ref.py), against answers written out by hand from the rule, and
against the outlines of utils/droplet_outlines.py, which it must invert; the readers' refusals and the label rule; compaction;
the script's flag on the CPU path and the refusals of both entry points.  Everything is exact equality."""
import json

import numpy as np
import pytest
from PIL import Image
from scipy import ndimage

from tests import polygon_cases as pc
from tests.test_confidence_cpu import files, run_script
from tests.test_outlines_cpu import random_labels
from utils import droplet_outlines as do
from utils import polygon_masks as pm


def fill(features, h, w, compact=False):
    return pm.rasterize_numpy(pm.pack(features), h, w, compact)


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_brute_force_on_random_polygons():
    hit = on_grid = 0
    for t, want in enumerate(pc.random_answers()):
        feats, h, w = pc.random_case(t)
        got = fill(feats, h, w)["labels"]
        assert got.dtype == np.int32 and np.array_equal(got, want), t
        hit += bool(want.any())
        on_grid += t % 3 == 0
    assert hit > 150 and on_grid == 67                       # the cases are not empty planes


@pytest.mark.parametrize("name", list(pc.known_answers()))
def test_known_answers(name):
    feats, h, w, want = pc.known_answers()[name]
    rec = fill(feats, h, w)
    assert rec["labels"].tolist() == want
    assert np.array_equal(rec["labels"], pc.polygon_ref.fill(feats, h, w))
    k = feats[0]["label"]
    n = int(np.count_nonzero(want))
    assert rec["kept"].tolist() == ([k] if n else []) and rec["area"].tolist() == ([n] if n else [])


def test_ring_orientation_and_start_do_not_matter():
    feats, h, w = pc.random_case(1)
    want = fill(feats, h, w)["labels"]
    ring = feats[0]["polygons"][0][0]
    for other in (ring[::-1], np.roll(ring, 2, axis=0)):
        again = [pc.feature(feats[0]["label"], [other] + feats[0]["polygons"][0][1:])]
        assert np.array_equal(fill(again, h, w)["labels"], want)


def test_quantisation_rounds_half_to_even_once():
    assert pm.quantise([0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256, 1.0, -3.25]).tolist() == [0, 2, 2, 0, 256, -832]
    assert [pc.polygon_ref.quantise(v) for v in (0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256)] == [0, 2, 2, 0]


# ---- round trips -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pc.round_trip_maps()))
def test_geojson_round_trip_is_the_identity(name):
    lab = pc.round_trip_maps()[name]
    doc = json.loads(json.dumps(do.geojson(do.outlines_numpy(lab), name)))
    feats = pm.features_of_geojson(doc)
    assert [f["label"] for f in feats] == [k for k in range(1, int(lab.max()) + 1) if (lab == k).any()]
    rec = fill(feats, *lab.shape)
    assert np.array_equal(rec["labels"], lab)
    assert np.array_equal(rec["area"], np.bincount(lab.ravel())[1:][np.bincount(lab.ravel())[1:] > 0])
    if name == "island in its hole":
        assert doc["features"][0]["geometry"]["type"] == "MultiPolygon"


def coco_expected(lab):
    """Per label and 4-connected piece: the piece filled against an 8-connected background; the larger label wins."""
    want = np.zeros(lab.shape, np.int64)
    for k in range(1, int(lab.max(initial=0)) + 1):
        pieces, n = ndimage.label(lab == k)
        for j in range(1, n + 1):
            want = np.maximum(want, ndimage.binary_fill_holes(pieces == j, structure=np.ones((3, 3))) * k)
    return want


def coco_doc(lab, name="im.png"):
    anns = do.coco_annotation(do.outlines_numpy(lab), image_id=1)
    return {"images": [{"id": 1, "file_name": name, "height": lab.shape[0], "width": lab.shape[1]}], "annotations": anns,
            "categories": [{"id": 1, "name": "droplet"}]}


def test_coco_round_trip_fills_the_holes_it_cannot_express():
    rng = np.random.default_rng(28)
    maps = list(pc.round_trip_maps().values())
    maps += [random_labels(int(h), int(w), 4000 + t, top=2) for t, (h, w) in enumerate(rng.integers(3, 20, size=(40, 2)))]
    holes = 0
    for lab in maps:
        by_stem = pm.images_of_coco(json.loads(json.dumps(coco_doc(lab))))
        feats, hw = by_stem["im"]
        assert hw == lab.shape
        want = coco_expected(lab)
        assert np.array_equal(fill(feats, *hw)["labels"], want)
        holes += not np.array_equal(want, lab)
    assert holes >= 5


# ---- readers ---------------------------------------------------------------------------------------------------------------------

def gj(*geoms, labels=None):
    labels = labels or [None] * len(geoms)
    return {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {} if k is None else {"label": k}, "geometry": g} for g, k in zip(geoms, labels)]}


POLY = {"type": "Polygon", "coordinates": [[[0, 0], [2, 0], [2, 2], [0, 2], [0, 0]]]}


def test_refusals():
    with pytest.raises(pm.PolygonError, match="ring of 2"):
        pm.pack(pm.features_of_geojson(gj({"type": "Polygon", "coordinates": [[[0, 0], [2, 0], [0, 0]]]})))
    with pytest.raises(pm.PolygonError, match="NaN"):
        pm.pack([pc.feature(1, [[(0, 0), (float("nan"), 1), (1, 1)]])])
    with pytest.raises(pm.PolygonError, match="NaN or infinite"):
        pm.pack([pc.feature(1, [[(0, 0), (float("inf"), 1), (1, 1)]])])
    with pytest.raises(pm.PolygonError, match="2\\^20"):
        pm.pack([pc.feature(1, [[(0, 0), (2 ** 20 + 1, 1), (1, 1)]])])
    pm.pack([pc.feature(1, [[(0, 0), (2 ** 20, -2 ** 20), (1, 1)]])])                 # the limit itself is legal
    with pytest.raises(pm.PolygonError, match="feature 1.*LineString"):
        pm.features_of_geojson(gj(POLY, {"type": "LineString", "coordinates": [[0, 0], [1, 1]]}), "f.geojson")
    img = {"images": [{"id": 1, "file_name": "a.png", "height": 4, "width": 4}]}
    rle = {"id": 7, "image_id": 1, "segmentation": {"counts": [0, 16], "size": [4, 4]}, "iscrowd": 1}
    with pytest.raises(pm.PolygonError, match="annotation 7.*RLE.*iscrowd"):
        pm.images_of_coco({**img, "annotations": [rle]})
    with pytest.raises(pm.PolygonError, match="RLE"):
        pm.images_of_coco({**img, "annotations": [{**rle, "iscrowd": 0, "segmentation": {"counts": "abc", "size": [4, 4]}}]})
    with pytest.raises(pm.PolygonError, match="label"):
        pm.pack([pc.feature(2 ** 31, [pc.SQUARE])])
    with pytest.raises(pm.PolygonError):
        pm.rasterize_numpy(pm.pack([]), 0, 4)
    with pytest.raises(pm.PolygonError):
        pm.rasterize_numpy(pm.pack([]), 16385, 4)


def test_closing_duplicate_is_dropped_and_the_record_is_plain():
    p = pm.pack(pm.features_of_geojson(gj(POLY, {"type": "MultiPolygon", "coordinates": [POLY["coordinates"], [[[3, 3], [5, 3], [4, 5]]]]})))
    assert p["verts"].dtype == p["ring_first"].dtype == p["poly_first_ring"].dtype == p["poly_label"].dtype == np.int32
    assert p["ring_first"].tolist() == [0, 4, 8, 11] and p["poly_first_ring"].tolist() == [0, 1, 2, 3] and p["poly_label"].tolist() == [1, 2, 2]
    assert p["verts"][:4].tolist() == [[0, 0], [512, 0], [512, 512], [0, 512]]
    empty = pm.pack([])
    assert empty["verts"].shape == (0, 2) and empty["ring_first"].tolist() == [0] and empty["poly_first_ring"].tolist() == [0]
    assert not pm.rasterize_numpy(empty, 3, 4)["labels"].any()


def test_label_rule():
    assert [f["label"] for f in pm.features_of_geojson(gj(POLY, POLY, labels=[7, 3]))] == [7, 3]
    assert [f["label"] for f in pm.features_of_geojson(gj(POLY, POLY, labels=[7, None]))] == [1, 2]       # one missing
    assert [f["label"] for f in pm.features_of_geojson(gj(POLY, POLY, labels=[7, 7]))] == [1, 2]          # not unique
    assert [f["label"] for f in pm.features_of_geojson(gj(POLY, POLY, labels=[7, 0]))] == [1, 2]          # not positive
    assert [f["label"] for f in pm.features_of_geojson(gj(POLY, POLY, labels=[7, 2.5]))] == [1, 2]        # not an integer
    img = {"images": [{"id": 1, "file_name": "d/a.tif", "height": 4, "width": 5}, {"id": 2, "file_name": "b.png", "height": 2, "width": 3}]}
    ann = lambda i, **kw: {"id": i, "image_id": 1, "segmentation": [[0, 0, 2, 0, 2, 2, 0, 2]], "iscrowd": 0, **kw}      # noqa: E731
    got = pm.images_of_coco({**img, "annotations": [ann(1, label=9), ann(2, label=4)]})
    assert [f["label"] for f in got["a"][0]] == [9, 4] and got["a"][1] == (4, 5)
    assert got["b"] == ([], (2, 3))                          # listed without annotations: an empty annotation
    assert [f["label"] for f in pm.images_of_coco({**img, "annotations": [ann(1, label=9), ann(2)]})["a"][0]] == [1, 2]


def test_overlap_union_and_compaction():
    big = [(0, 0), (6, 0), (6, 6), (0, 6)]
    feats = [pc.feature(5, [big]), pc.feature(9, [[(0.1, 0.1), (0.4, 0.1), (0.1, 0.4)]]), pc.feature(12, [[(2, 2), (4, 2), (4, 4), (2, 4)]])]
    rec = fill(feats, 6, 7, compact=True)
    want = np.zeros((6, 7), np.int32)
    want[:6, :6] = 1
    want[2:4, 2:4] = 2
    assert np.array_equal(rec["labels"], want) and rec["kept"].tolist() == [5, 12]
    assert np.array_equal(rec["area"], np.bincount(want.ravel())[1:]) and rec["kept"].dtype == rec["area"].dtype == np.int64
    plain = fill(feats, 6, 7)
    assert sorted(np.unique(plain["labels"])) == [0, 5, 12] and plain["kept"].tolist() == [5, 12]
    assert np.array_equal(fill(feats[::-1], 6, 7)["labels"], plain["labels"])        # independent of the order
    # a feature that loses every pixel to a larger label is dropped as well
    lost = fill([pc.feature(3, [[(2, 2), (4, 2), (4, 4), (2, 4)]]), pc.feature(8, [big])], 6, 7, compact=True)
    assert lost["kept"].tolist() == [8] and lost["labels"].max() == 1
    # the polygons of one feature union: an island inside another part's hole, and two overlapping parts (per-feature XOR
    # would clear the overlap)
    two = fill([pc.feature(2, [[(0, 0), (3, 0), (3, 3), (0, 3)]], [[(1, 1), (5, 1), (5, 5), (1, 5)]])], 6, 7)["labels"]
    want = np.zeros((6, 7), np.int32)
    want[:3, :3] = want[1:5, 1:5] = 2
    assert np.array_equal(two, want)


# ---- the scripts -----------------------------------------------------------------------------------------------------------------

SIZES = ((48, 48), (40, 56))


def polygon_arms(tmp_path, monkeypatch, device="cpu"):
    """A run with --outlines at another threshold writes the annotation; then the polygon arm and its yardstick, --gt_dir with
    --gt_labels on the label images the same files fill to on the host."""
    src = run_script(tmp_path, monkeypatch, "src", ["--outlines", "--prob_thresh", "0.45"], device=device, sizes=SIZES)
    gtd = tmp_path / "gt_png"
    gtd.mkdir()
    for i, hw in enumerate(SIZES):
        rec = pm.rasterize_numpy(pm.pack(pm.read_geojson(src / "outlines" / f"im{i}.geojson")), *hw, compact=True)
        assert rec["labels"].max() >= 2
        Image.fromarray(rec["labels"].astype(np.uint16)).save(gtd / f"im{i}.png")
    extra = ["--thresh_sweep", "10", "--boundary", "8", "--diff_maps"]
    poly = run_script(tmp_path, monkeypatch, "poly", ["--gt_polygons", str(src / "outlines")] + extra, device=device, sizes=SIZES)
    png = run_script(tmp_path, monkeypatch, "png", ["--gt_dir", str(gtd), "--gt_labels"] + extra, device=device, sizes=SIZES)
    return src, poly, png


def test_script_cpu_path_equals_the_label_image_arm(tmp_path, monkeypatch, capsys):
    src, poly, png = polygon_arms(tmp_path, monkeypatch)
    assert "--gt_polygons: 0 of" in capsys.readouterr().out
    assert files(poly) == files(png) and {"gt_droplets.csv", "match_per_image.csv", "threshold_sweep.csv", "boundary_per_image.csv",
                                           "diff_regions.csv"} <= set(files(poly))
    for f in files(poly):
        assert (poly / f).read_bytes() == (png / f).read_bytes(), f
    # a COCO file of the same annotation serves as well (these droplets have no holes to lose)
    coco = run_script(tmp_path, monkeypatch, "coco", ["--gt_polygons", str(src / "outlines_coco.json")], sizes=SIZES)
    plain = run_script(tmp_path, monkeypatch, "poly2", ["--gt_polygons", str(src / "outlines")], sizes=SIZES)
    for f in ("gt_droplets.csv", "match_per_image.csv", "all_droplets.csv"):
        assert (coco / f).read_bytes() == (plain / f).read_bytes(), f


def test_quantify_refusals_come_before_any_image(tmp_path, monkeypatch):
    import quantify_droplets_batch as q
    src = run_script(tmp_path, monkeypatch, "src", ["--outlines"], sizes=SIZES)
    with pytest.raises(SystemExit) as e:
        run_script(tmp_path, monkeypatch, "both", ["--gt_polygons", str(src / "outlines"), "--gt_dir", str(src / "predicted_masks")], sizes=SIZES)
    assert e.value.code == 2 and not (tmp_path / "both").exists()
    (src / "outlines" / "im1.geojson").unlink()
    monkeypatch.setattr(q, "load_model", None)               # never reached
    with pytest.raises(SystemExit) as e:
        run_script_keeping_model(tmp_path, monkeypatch, q, "missing", ["--gt_polygons", str(src / "outlines")])
    assert "--gt_polygons: no polygon file for im1.png" in str(e.value.code) and not (tmp_path / "missing").exists()
    coco = json.loads((src / "outlines_coco.json").read_text())
    coco["images"][0]["width"] += 1
    (tmp_path / "bad.json").write_text(json.dumps(coco))
    with pytest.raises(SystemExit) as e:
        run_script_keeping_model(tmp_path, monkeypatch, q, "size", ["--gt_polygons", str(tmp_path / "bad.json")])
    assert "--gt_polygons" in str(e.value.code) and "49 x 48" in str(e.value.code) and not (tmp_path / "size").exists()
    for flag in (["--thresh_sweep"], ["--boundary"]):        # without either source the old words stay
        with pytest.raises(SystemExit) as e:
            run_script_keeping_model(tmp_path, monkeypatch, q, "none", flag)
        assert "it needs --gt_dir" in str(e.value.code)


def run_script_keeping_model(tmp_path, monkeypatch, q, tag, extra):
    """run_script's command line without its patches: load_model stays what the caller set (None: it must not be reached)."""
    return q.main(["--img_dir", str(tmp_path / "imgs"), "--out_dir", str(tmp_path / tag), "--batch", "2", "--skip_excel", "--skip_histogram",
                   "--background_radius", "15", "--prob_thresh", "0.3", "--min_area", "2", *extra])


def test_train_refusals_come_before_any_file_is_read(tmp_path):
    import train_DC_focal
    missing = str(tmp_path / "no_such_dir")
    base = ["--image_dir", missing, "--ckpt_path", str(tmp_path / "ck.pth")]
    with pytest.raises(SystemExit) as e:
        train_DC_focal.main(base + ["--mask_polygons", missing])
    assert isinstance(e.value.code, str) and "--mask_polygons needs --device_data" in e.value.code
    with pytest.raises(SystemExit) as e:
        train_DC_focal.main(base + ["--mask_polygons", missing, "--mask_dir", missing, "--device_data"])
    assert isinstance(e.value.code, str) and "--mask_polygons and --mask_dir" in e.value.code
    assert train_DC_focal.build_parser().parse_args([]).mask_polygons is None
