"""CPU: the difference map and its 8-connected regions.  utils/difference_map.py against the plain
loops of tests/diffmap_ref.py, the colours against the table of the definition and the reference's colour thresholds, the
refusals of the two C entry points with host memory standing in, --diff_maps of both scripts on the CPU path."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from tests import diffmap_ref as R
from tests.test_split_cpu import SIZE, FixedProbs, cli_probs, files, run_cli
from utils import difference_map as D


@pytest.mark.parametrize("name", sorted(R.small_cases()))
def test_host_path_equals_plain_loops(name):
    pred, gt = R.small_cases()[name]
    assert D.class_plane(pred, gt).tolist() == R.class_plane_ref(pred.tolist(), gt.tolist())
    for min_area in (1, 5):
        assert R.record_as_ref(D.diff_regions_numpy(pred, gt, min_area)) == R.regions_ref(pred.tolist(), gt.tolist(), min_area), min_area


def test_connectivity_is_eight():
    """Cases a 4-connected labelling gets wrong."""
    for h, w in [(2, 2), (37, 53)]:
        im = D.diff_regions_numpy(*R.checkerboard(h, w, 1, 2))["image"]
        assert im[4:8].tolist() == [0, 1, 1, 0], (h, w)
    rec = D.diff_regions_numpy(*R.from_classes([[3, 2], [2, 3]]))
    assert rec["image"][4:8].tolist() == [0, 0, 1, 1] and rec["area"].tolist() == [2, 2] and rec["class"].tolist() == [3, 2]
    assert rec["neighbors"].tolist() == [1 << 2, 1 << 3]
    for k in (1, 2, 3):
        rec = D.diff_regions_numpy(*R.anti_diagonal(96, 130, k, 0))
        assert rec["image"][4 + k] == 1 and rec["area"].tolist() == [96] and rec["neighbors"].tolist() == [1]
    assert D.diff_regions_numpy(*R.serpentine())["image"][4:8].tolist() == [1, 0, 0, 1]
    assert D.diff_regions_numpy(*R.four_class_tiles(), 2)["image"].tolist() == [1024] * 8 + [0] * 4


def test_colours_are_the_table_and_the_reference_thresholds_select_the_classes():
    rng = np.random.default_rng(3)
    pred, gt = R.from_classes(rng.integers(0, 4, (37, 53)))
    pred, gt = pred * 200, gt * 3                                      # nonzero counts as 1
    c = D.class_plane(pred, gt)
    rgb = D.difference_map_rgb(pred, gt)
    assert rgb.dtype == np.uint8 and rgb.shape == (37, 53, 3)
    for k, colour in {0: (0, 0, 0), 1: (0, 255, 0), 2: (255, 0, 0), 3: (255, 255, 0)}.items():
        assert (c == k).any() and np.all(rgb[c == k] == np.array(colour, np.uint8)), k
    assert [[tuple(px) for px in row] for row in rgb.tolist()] == R.colors_ref(c.tolist())
    r, g, b = (rgb[:, :, j].astype(int) for j in range(3))
    assert np.array_equal((r > 200) & (g > 200) & (b < 50), c == 3)                     # yellow
    assert np.array_equal((r > 200) & (g < 50) & (b < 50), c == 2)                      # red
    assert np.array_equal((r < 50) & (g > 200) & (b < 50), c == 1)                      # green
    assert np.array_equal((r < 50) & (g < 50) & (b < 50), c == 0)                       # black
    image = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    over = D.overlay_difference(image, pred, gt)
    assert [[tuple(px) for px in row] for row in over.tolist()] == R.overlay_ref(image.tolist(), c.tolist())
    assert np.array_equal(over[c == 0], image[c == 0]) and np.array_equal(over[c != 0], rgb[c != 0])


def test_tables():
    pred, gt = R.small_cases()["realistic_moved/96x130"]
    rec = D.diff_regions_numpy(pred, gt, 3)
    t = D.region_table("a.png", rec, 2.0)
    assert list(t) == ["filename", "class", "area", "centroid-0", "centroid-1", "touches_common", "isolated", "area_sqmicron"]
    assert list(D.region_table("a.png", rec))[-1] == "isolated" and set(t["class"]) <= {"green", "red", "yellow"}
    assert np.array_equal(t["centroid-0"], rec["sumy"] / rec["area"]) and np.array_equal(t["area_sqmicron"], rec["area"] / 4.0)
    yellow = rec["class"] == D.YELLOW
    assert not t["touches_common"][yellow].any() and not t["isolated"][yellow].any()
    assert np.array_equal(t["isolated"][~yellow], ~t["touches_common"][~yellow])
    cols = D.image_columns(rec)
    assert tuple(cols) == D.IMAGE_COLUMNS and D.IMAGE_COLUMNS[:4] == ("yellow_blobs", "red_blobs", "green_blobs", "black_blobs")
    assert cols["red_kept"] == int((rec["class"] == D.RED).sum()) and cols["black_px"] == int(((pred == 0) & (gt == 0)).sum())
    assert cols["missed_droplets"] == int((t["isolated"] & (rec["class"] == D.RED)).sum())
    # a droplet missed entirely and a spurious one, next to one that was found with a rim
    gt = np.zeros((40, 60), np.uint8)
    pred = gt.copy()
    gt[5:15, 5:15], gt[25:35, 5:15] = 1, 1
    pred[5:15, 6:16], pred[25:35, 40:50] = 1, 1
    cols = D.image_columns(D.diff_regions_numpy(pred, gt))
    assert (cols["yellow_blobs"], cols["red_blobs"], cols["green_blobs"], cols["black_blobs"]) == (1, 2, 2, 1)
    assert cols["missed_droplets"] == 1 and cols["spurious_droplets"] == 1
    assert D.sum_image_columns([cols, cols])["red_blobs"] == 4 and set(D.sum_image_columns([]).values()) == {0}


# ---- the C entry points, host side -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def formula(h, w):
    n = h * w
    return 29 * n + 4 * ((n + 1023) // 1024) + 128


def test_workspace_query_is_the_documented_formula(lib):
    for h, w in [(1, 1), (1, 64), (37, 53), (96, 130), (1040, 1388), (16384, 16384)]:
        assert lib.unetdc_diff_regions_workspace(h, w) == formula(h, w), (h, w)
    for h, w in [(0, 5), (5, 0), (-1, 5), (16385, 5), (5, 16385), (32768, 32768)]:
        assert lib.unetdc_diff_regions_workspace(h, w) == 0, (h, w)


def test_abi_refusals_before_any_launch(lib):
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every check below fails before any HIP call

    def regions(pred=fake, gt=fake, h=64, w=64, min_area=1, ws=fake, bytes_=1 << 40, image=fake, count=fake, table=fake, max_out=10):
        return lib.unetdc_diff_regions(pred, gt, h, w, min_area, ws, bytes_, image, count, table, table, table, table, table,
                                       max_out, None)
    for kw, msg in [(dict(pred=None), b"null"), (dict(gt=None), b"null"), (dict(ws=None), b"null"), (dict(image=None), b"null"),
                    (dict(count=None), b"null"), (dict(table=None), b"null"), (dict(h=0), b"geometry"), (dict(w=0), b"geometry"),
                    (dict(h=-3), b"geometry"), (dict(w=16385), b"geometry"), (dict(h=16385), b"geometry"),
                    (dict(min_area=0), b"geometry"), (dict(max_out=-1), b"geometry"),
                    (dict(ws=ctypes.c_void_p(4100)), b"aligned"), (dict(image=ctypes.c_void_p(4100)), b"aligned"),
                    (dict(count=ctypes.c_void_p(4098)), b"aligned"), (dict(table=ctypes.c_void_p(4100)), b"aligned")]:
        assert regions(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    # h * w >= 2^30 cannot be reached with sides of at most 16384 (2^28): the limit is the sides'; the query refuses alike
    assert lib.unetdc_diff_regions_workspace(32768, 32768) == 0 and regions(h=32768, w=32768) == -1
    rc = regions(h=37, w=53, bytes_=formula(37, 53) - 1)
    err = lib.unetdc_last_error()
    assert rc == -3 and err.startswith(b"diff_regions") and b"workspace too small" in err, (rc, err)

    def paint(pred=fake, gt=fake, rgb=fake, h=64, w=64, diff=fake, over=fake):
        return lib.unetdc_diff_paint(pred, gt, rgb, h, w, diff, over, None)
    for kw, msg in [(dict(pred=None), b"null"), (dict(gt=None), b"null"), (dict(h=0), b"geometry"), (dict(w=16385), b"geometry"),
                    (dict(rgb=None), b"needs rgb"), (dict(diff=None, over=None), b"no output")]:
        assert paint(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())


# ---- quantify_droplets_batch.py --diff_maps on the CPU path -----------------------------------------------------------------
DIFF_FILES = (["diff_regions.csv", "diff_regions_per_image.csv"] + [f"difference_maps/im{i}_diffmap.png" for i in range(3)] +
              [f"diff_overlays/im{i}_overlay.png" for i in range(3)])


def cli_gt_dir(tmp_path):
    from tests.test_match_cpu import cli_gt_masks, write_gt
    d = tmp_path / "gt"
    return d if d.exists() else write_gt(d, cli_gt_masks(), scale=200)


def test_cli_diff_maps_on_the_cpu_path(tmp_path, monkeypatch):
    from tests.test_match_cpu import cli_gt_masks
    gt_dir = cli_gt_dir(tmp_path)
    base = ["--gt_dir", str(gt_dir), "--save_overlays", "--density_maps"]
    plain = run_cli(tmp_path, monkeypatch, "plain", base)
    out = run_cli(tmp_path, monkeypatch, "diff", base + ["--diff_maps"])
    assert sorted(set(files(out)) - set(files(plain))) == sorted(DIFF_FILES)
    for f in files(plain):                                             # every file of the run without the flag: byte for byte
        assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    regions = pd.read_csv(out / "diff_regions.csv", float_precision="round_trip")
    per_image = pd.read_csv(out / "diff_regions_per_image.csv")
    assert list(regions.columns) == ["filename", "class", "area", "centroid-0", "centroid-1", "touches_common", "isolated"]
    assert list(per_image.columns) == ["filename"] + list(D.IMAGE_COLUMNS) and per_image["filename"].tolist() == [f"im{i}.png" for i in range(3)]
    gts = cli_gt_masks()
    for i in range(3):
        pred = (cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8)
        rgb = np.array(Image.open(tmp_path / "imgs" / f"im{i}.png").convert("RGB"))
        assert np.array_equal(np.array(Image.open(out / "difference_maps" / f"im{i}_diffmap.png")), D.difference_map_rgb(pred, gts[i]))
        assert np.array_equal(np.array(Image.open(out / "diff_overlays" / f"im{i}_overlay.png")), D.overlay_difference(rgb, pred, gts[i]))
        image, rows = R.regions_ref(pred.tolist(), gts[i].tolist())
        got = regions[regions["filename"] == f"im{i}.png"]
        assert got["area"].tolist() == [r[1] for r in rows] and got["class"].tolist() == [D.CLASS_NAMES[r[0]] for r in rows]
        assert got["touches_common"].tolist() == [bool(r[4] >> 3 & 1) for r in rows]
        assert got["centroid-1"].tolist() == [r[3] / r[1] for r in rows]
        r = per_image.iloc[i]
        assert [int(r[q]) for q in D.IMAGE_COLUMNS[:4]] == [image[4 + k] for k in (3, 2, 1, 0)]
    assert per_image["missed_droplets"][2] == 1 and per_image["yellow_blobs"][2] == 0   # image 2: nothing predicted, one square annotated
    # MIN_AREA drops rows and kept counts, never the reference's four counts
    big = run_cli(tmp_path, monkeypatch, "big", base + ["--diff_maps", "30"])
    per_big = pd.read_csv(big / "diff_regions_per_image.csv")
    assert per_big[list(D.IMAGE_COLUMNS[:8])].equals(per_image[list(D.IMAGE_COLUMNS[:8])])
    assert len(pd.read_csv(big / "diff_regions.csv")) < len(regions) and pd.read_csv(big / "diff_regions.csv")["area"].min() >= 30


def test_cli_diff_maps_needs_gt_dir_and_a_positive_area(tmp_path, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        run_cli(tmp_path, monkeypatch, "nogt", ["--diff_maps"])
    assert e.value.code == 2 and "--gt_dir" in capsys.readouterr().err and not (tmp_path / "nogt").exists()
    with pytest.raises(SystemExit) as e:
        run_cli(tmp_path, monkeypatch, "zero", ["--gt_dir", str(cli_gt_dir(tmp_path)), "--diff_maps", "0"])
    assert e.value.code == 2 and not (tmp_path / "zero").exists()


# ---- train_DC_focal.py --diff_maps ---------------------------------------------------------------------------------------------
def evaluate_fixed(out_dir, device):
    """evaluate_test(diff_maps=out_dir) on fixed probabilities: two batches, the first with file names as the loaders yield them,
    the second without.  -> {"record", "files"}."""
    import train_DC_focal as T
    from tests.test_match_cpu import cli_gt_masks
    probs = cli_probs()
    rng = np.random.default_rng(4)
    images = torch.from_numpy(rng.random((3, 3, SIZE, SIZE)).astype(np.float32))
    masks = torch.from_numpy(np.stack(cli_gt_masks()).astype(np.float32))[:, None]
    loader = [(images[:2], masks[:2], [(SIZE, SIZE)] * 2, ["first.png", "second.tif"]), (images[2:], masks[2:])]
    rec = T.evaluate_test(FixedProbs(probs), loader, lambda o, m: (o - m).abs().mean(), torch.device(device), diff_maps=str(out_dir))
    return {"record": rec, "files": files(out_dir), "images": images, "masks": masks, "probs": probs}


def test_evaluate_test_diff_maps_on_the_cpu(tmp_path):
    import train_DC_focal as T
    from tests.test_match_cpu import cli_gt_masks
    run = evaluate_fixed(tmp_path / "dumps", "cpu")
    names = ["first", "second", "test_00002"]
    assert run["files"] == sorted([f"differences_map_test/{n}_diffmap.png" for n in names] + [f"overlay_diff_test/{n}_overlay.png" for n in names])
    rows = []
    for i, n in enumerate(names):
        pred, gt = (run["probs"][i, 0].numpy() > 0.3).astype(np.uint8), cli_gt_masks()[i]
        rgb = (run["images"][i].numpy().transpose(1, 2, 0) * 255).astype(np.uint8)      # truncating
        assert np.array_equal(np.array(Image.open(tmp_path / "dumps" / "differences_map_test" / f"{n}_diffmap.png")),
                              D.difference_map_rgb(pred, gt))
        assert np.array_equal(np.array(Image.open(tmp_path / "dumps" / "overlay_diff_test" / f"{n}_overlay.png")),
                              D.overlay_difference(rgb, pred, gt))
        rows.append(D.image_columns(D.diff_regions_numpy(pred, gt)))
    assert run["record"]["diff_regions"] == D.sum_image_columns(rows) and run["record"]["diff_regions"]["yellow_blobs"] > 0
    plain = T.evaluate_test(FixedProbs(run["probs"]), [(run["images"], run["masks"])], lambda o, m: (o - m).abs().mean(),
                            torch.device("cpu"))
    assert "diff_regions" not in plain and plain["confusion"] == run["record"]["confusion"]


def test_train_synthetic_with_diff_maps_on_the_cpu(tmp_path, capsys):
    import train_DC_focal as T
    args = ["--synthetic", "--synthetic_len", "10", "--img_size", "32", "--batch", "2", "--epochs", "1", "--steps", "1",
            "--workers", "0", "--device", "cpu", "--ckpt_path", str(tmp_path / "m.pth")]
    hist = T.main(args + ["--diff_maps", str(tmp_path / "dumps")])
    d = hist.test["diff_regions"]
    assert tuple(d) == D.IMAGE_COLUMNS and d["black_px"] + d["green_px"] + d["red_px"] + d["yellow_px"] == 2 * 32 * 32
    got = files(tmp_path / "dumps")                                    # the synthetic tiles carry names: synthetic_%05d
    stems = sorted(os.path.basename(f)[:-len("_diffmap.png")] for f in got if f.startswith("differences_map_test/"))
    assert len(stems) == 2 and all(s.startswith("synthetic_") for s in stems)
    assert got == sorted([f"differences_map_test/{s}_diffmap.png" for s in stems] + [f"overlay_diff_test/{s}_overlay.png" for s in stems])
    assert "Difference maps under" in capsys.readouterr().out
    assert T.build_parser().parse_args(["--diff_maps"]).diff_maps == "." and T.build_parser().parse_args([]).diff_maps is None
    import train
    assert train.build_parser(arch="unet").parse_args(["--diff_maps", "x"]).diff_maps == "x"
    with pytest.raises(SystemExit, match="--in_channels 1"):
        T.main(args + ["--diff_maps", "--in_channels", "1"])
    assert "diff_regions" not in T.main(args).test and set(os.listdir(tmp_path)) <= {"dumps", "m.pth"}
