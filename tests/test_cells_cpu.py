"""CPU: droplets per cell.  utils/droplet_cells.py -- the path the script takes without a GPU and the
yardstick of csrc/cells.hip -- against the brute-force oracle of tests/cells_ref.py; the host-side argument checks of the four
C ABI entries (no launch: host memory stands in for device memory); the script's flags, columns and files on the CPU path."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from tests import cells_ref as ref
from utils import droplet_cells as dc

EDT_INF = 2 ** 31 - 1


def assert_nearest_equals_brute(label, max_label, radius=0):
    got, want = dc.nearest_label_numpy(label, max_label, radius), ref.nearest_brute(label, max_label, radius)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


# ---- nearest label ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.nearest_cases()))
def test_nearest_label_equals_brute_force(name):
    label, max_label = ref.nearest_cases()[name]
    assert_nearest_equals_brute(label, max_label)


def test_row_tie_takes_the_smaller_label():
    """1 x 7, label 2 at the left end and label 1 at the right: the centre pixel ties at 9 and takes label 1 -- a row scan that
    stops at dx^2 >= best (the rule of the plain distance transform) never sees the seed on the right."""
    lab, d2 = assert_nearest_equals_brute(*ref.nearest_cases()["row_tie"])
    assert lab.tolist() == [[2, 2, 2, 1, 1, 1, 1]] and d2.tolist() == [[0, 1, 4, 9, 4, 1, 0]]


def test_column_tie_takes_the_smaller_label():
    lab, d2 = assert_nearest_equals_brute(*ref.nearest_cases()["column_tie"])
    assert (lab[0:2] == 5).all() and (lab[2:5] == 2).all()
    assert d2[:, 3].tolist() == [0, 1, 4, 1, 0]


def test_random_seeds_exercise_the_tie_rule_and_match_scipy_distances():
    from scipy import ndimage
    label, max_label = ref.nearest_cases()["random_seeds"]
    lab, d2 = assert_nearest_equals_brute(label, max_label)
    idx = ndimage.distance_transform_edt(label == 0, return_indices=True)[1]
    differs = int((label[idx[0], idx[1]] != lab).sum())
    print(f"[cells] SciPy's index pick differs from the tie rule on {differs} pixels")
    assert differs > 0                                   # the tie rule is exercised
    yy, xx = np.mgrid[0:label.shape[0], 0:label.shape[1]]
    assert np.array_equal(d2, (yy - idx[0]) ** 2 + (xx - idx[1]) ** 2)


@pytest.mark.parametrize("radius", [1, 3, 0])
def test_radius_zeroes_the_label_and_keeps_the_distance(radius):
    label, max_label = ref.nearest_cases()["random_seeds"]
    free = dc.nearest_label_numpy(label, max_label, 0)
    lab, d2 = assert_nearest_equals_brute(label, max_label, radius)
    assert np.array_equal(d2, free[1])
    cut = d2 > radius * radius if radius else np.zeros_like(d2, bool)
    assert (lab[cut] == 0).all() and np.array_equal(lab[~cut], free[0][~cut]) and (free[0] > 0).all()
    assert cut.any() == (radius > 0)


def test_no_seed_all_seeds_and_out_of_range_labels():
    cases = ref.nearest_cases()
    lab, d2 = dc.nearest_label_numpy(*cases["no_seed"])
    assert (lab == 0).all() and (d2 == EDT_INF).all()
    label, max_label = cases["all_seeds"]
    lab, d2 = dc.nearest_label_numpy(label, max_label)
    assert np.array_equal(lab, label) and (d2 == 0).all()
    label, max_label = cases["out_of_range"]
    lab, d2 = dc.nearest_label_numpy(label, max_label)
    for y, x in ((2, 3), (7, 9), (10, 16)):              # not seeds: they take a neighbour's label at a positive distance
        assert d2[y, x] > 0 and 1 <= lab[y, x] <= max_label
    assert set(np.unique(lab)) <= set(range(1, max_label + 1))
    # with max_label = 0 nothing is a seed
    lab, d2 = dc.nearest_label_numpy(label, 0)
    assert (lab == 0).all() and (d2 == EDT_INF).all()


def test_micrograph_size_takes_seconds():
    import time
    rng = np.random.default_rng(3)
    label = np.zeros((1040, 1388), np.int32)
    for k in range(50):
        y, x = rng.integers(20, 1020), rng.integers(20, 1368)
        label[y - 12:y + 12, x - 12:x + 12] = k + 1
    t = time.time()
    lab, d2 = dc.nearest_label_numpy(label, 50)
    took = time.time() - t
    print(f"[cells] nearest_label_numpy at 1040 x 1388, 50 nuclei: {took:.1f} s")
    assert took < 600 and (lab > 0).all()                # seconds on an idle host (about 5); the bound only catches a quadratic path and np.array_equal(lab[label > 0], label[label > 0])
    rows = rng.integers(0, 1040, 2)                      # a few whole rows against the brute force
    want = ref.nearest_brute(label, 50, rows=rows)
    assert np.array_equal(lab[rows], want[0]) and np.array_equal(d2[rows], want[1])


# ---- cell table -------------------------------------------------------------------------------------------------------------------
def table_d2(cell, max_cell):
    """A d2 plane for the table cases: the distance to the 2 x 2 'nucleus' at the first pixels of every cell."""
    nuc = np.zeros_like(cell)
    for k in range(1, max_cell + 1):
        ys, xs = np.nonzero(cell == k)
        if len(ys):
            nuc[ys[0]:ys[0] + 2, xs[0]:xs[0] + 2] = k
    return ref.nearest_brute(nuc, max(max_cell, 1))[1]


@pytest.mark.parametrize("with_d2", [False, True])
@pytest.mark.parametrize("name", sorted(ref.table_cases()))
def test_cell_table_equals_brute_force(name, with_d2):
    drop, md, cell, mc = ref.table_cases()[name]
    d2 = table_d2(cell, 5) if with_d2 else None
    got, want = dc.cell_table_numpy(drop, md, cell, mc, d2), ref.cell_table_brute(drop, md, cell, mc, d2)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[0].shape == (6, md) and got[1].shape == (8, mc)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_cell_table_cases_by_hand():
    drop, md, cell, mc = ref.table_cases()["mixed"]
    d2 = table_d2(cell, mc)
    out_d, out_c, needed = dc.cell_table_numpy(drop, md, cell, mc, d2)
    D = {q: out_d[j] for j, q in enumerate(dc.DROPLET_QUANTITIES)}
    C = {q: out_c[j] for j, q in enumerate(dc.CELL_QUANTITIES)}
    assert (D["cell"][0], D["n_in"][0], D["n_cells"][0], D["n_out"][0], D["area"][0]) == (1, 6, 1, 0, 6)     # wholly inside cell 1
    assert (D["cell"][2], D["n_in"][2], D["n_cells"][2]) == (2, 3, 2)                      # 3 / 3 between cells 4 and 2
    assert (D["cell"][3], D["n_in"][3], D["n_cells"][3], D["n_out"][3]) == (0, 0, 0, D["area"][3])           # outside any cell
    assert (D["cell"][4], D["n_in"][4], D["n_cells"][4]) == (3, 3, 3)                      # over three cells
    assert (D["cell"][5], D["n_out"][5]) == (0, 4)                                         # on a cell label above max_cell
    assert D["area"][6] == 0 and D["min_d2"][6] == EDT_INF and D["cell"][6] == 0           # a label without a pixel
    assert C["n_border"][0] == 11 and (C["n_border"][1:] == 0).all()                       # cell 1 lies in the corner
    assert C["n_droplets"].tolist() == [1, 1, 1, 1, 0] and C["max_area"][4] == 0           # cell 5 has no droplet
    assert C["fg_px"][0] == 6 and C["S_area2"][3] == 25 and needed == 8
    assert (C["nucleus_px"] == 4).all() and D["min_d2"][0] == 0 and D["min_d2"][3] > 0
    none = dc.cell_table_numpy(drop, md, cell, mc, None)
    assert (none[0][5] == EDT_INF).all() and (none[1][7] == 0).all()
    assert np.array_equal(none[0][:5], out_d[:5]) and np.array_equal(none[1][:7], out_c[:7])


# ---- C ABI: argument checks before any launch --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def check_refusals(lib, a):
    """Every documented refusal of the four entries, with `a` standing for every pointer (64-byte aligned; nothing may be
    launched on it): -1 or -3 and a message that names the stage; the queries answer 0 for what the calls refuse."""
    assert lib.unetdc_label_nearest_workspace(37, 53) >= 2 * 4 * 37 * 53
    for hw in ((0, 5), (5, 0), (-1, 5), (16385, 5), (5, 16385)):
        assert lib.unetdc_label_nearest_workspace(*hw) == 0 and lib.unetdc_cell_table_workspace(*hw, 3, 3, 8) == 0
    assert lib.unetdc_label_nearest_workspace(16384, 16384) == 2 * 4 * 16384 * 16384
    for args in ((64, 64, -1, 3, 8), (64, 64, 3, -1, 8), (64, 64, 3, 3, -1)):
        assert lib.unetdc_cell_table_workspace(*args) == 0

    def nearest(label=a, max_label=3, h=8, w=8, radius=0, ws=a, nbytes=1 << 30, out_label=a, out_d2=a):
        return lib.unetdc_label_nearest(label, max_label, h, w, radius, ws, nbytes, out_label, out_d2, None)
    for kw in (dict(label=None), dict(ws=None), dict(out_label=None), dict(out_d2=None), dict(h=0), dict(w=0), dict(h=16385),
               dict(w=16385), dict(radius=-1), dict(radius=32768), dict(max_label=-1)):
        assert nearest(**kw) == -1 and lib.unetdc_last_error().startswith(b"label_nearest"), (kw, lib.unetdc_last_error())
    need = lib.unetdc_label_nearest_workspace(8, 8)
    assert nearest(nbytes=need - 1) == -3 and lib.unetdc_last_error().startswith(b"label_nearest: workspace too small")

    def table(drop=a, md=3, cell=a, mc=3, h=8, w=8, ws=a, nbytes=1 << 30, needed=a, room=8, out_d=a, out_c=a):
        return lib.unetdc_cell_table(drop, md, cell, mc, None, h, w, ws, nbytes, needed, room, out_d, out_c, None)
    for kw in (dict(drop=None), dict(cell=None), dict(ws=None), dict(needed=None), dict(out_d=None), dict(out_c=None), dict(h=0),
               dict(w=16385), dict(md=-1), dict(mc=-1), dict(room=-1)):
        assert table(**kw) == -1 and lib.unetdc_last_error().startswith(b"cell_table"), (kw, lib.unetdc_last_error())
    need = lib.unetdc_cell_table_workspace(8, 8, 3, 3, 8)
    assert need > 0 and table(nbytes=need - 1) == -3 and lib.unetdc_last_error().startswith(b"cell_table: workspace too small")


def test_abi_refusals_come_before_any_launch(lib):
    buf = ctypes.create_string_buffer(4096)
    check_refusals(lib, (ctypes.addressof(buf) + 63) // 64 * 64)


# ---- the script on the CPU path ---------------------------------------------------------------------------------------------------
SIZES = ((64, 64), (48, 80))
NEW_DROPLET_COLUMNS = ["cell", "cell_overlap_frac", "n_cells", "outside_cells"]
SUMMARY_COLUMNS = list(dc.SUMMARY_NAMES)


def cli_probs():
    from tests.test_split_cpu import cli_probs as three
    return three()[:2]


def write_masks(d, sizes=SIZES, as_labels=False):
    """Per image three rectangular 'nuclei' (or, as labels, the same rectangles numbered 3, 1, 2 in a 16-bit image)."""
    d.mkdir()
    maps = []
    for i, (h, w) in enumerate(sizes):
        m = np.zeros((h, w), np.int32)
        m[4:10, 5:12], m[h // 2:h // 2 + 5, w // 2:w // 2 + 6], m[h - 9:h - 3, 8:15] = 3, 1, 2
        maps.append(m)
        Image.fromarray(m.astype(np.uint16) if as_labels else ((m > 0) * 255).astype(np.uint8)).save(d / f"im{i}.png")
    return maps


def run(tmp_path, monkeypatch, tag, extra, device="cpu"):
    from tests.test_split_cpu import run_cli
    return run_cli(tmp_path, monkeypatch, tag, ["--px_per_micron", "2.0", *extra], device=device, sizes=SIZES, probs=cli_probs())


def test_cli_cells_and_nuclei_on_the_cpu_path(tmp_path, monkeypatch):
    from scipy import ndimage
    from tests.test_split_cpu import files
    write_masks(tmp_path / "nuc")
    labelled = write_masks(tmp_path / "lab", as_labels=True)
    plain = run(tmp_path, monkeypatch, "plain", [])
    cells = run(tmp_path, monkeypatch, "cells", ["--cell_dir", str(tmp_path / "lab"), "--cell_labels"])
    nuclei = run(tmp_path, monkeypatch, "nuclei", ["--nuclei_dir", str(tmp_path / "nuc"), "--cell_radius", "20"])
    # the new files, and nothing else changes: the plain run's files are there byte for byte but for the tables that gain columns
    assert sorted(set(files(cells)) - set(files(plain))) == ["cells.csv", "cells_per_image.csv"]
    assert sorted(set(files(nuclei)) - set(files(plain))) == ["cell_territories/im0_cells.png", "cell_territories/im1_cells.png", "cells.csv",
                                                              "cells_per_image.csv"]
    grown = {"all_droplets.csv", "im0_droplets.csv", "im1_droplets.csv", "summary_per_image.csv"}
    for f in files(plain):
        assert f in grown or (plain / f).read_bytes() == (cells / f).read_bytes() == (nuclei / f).read_bytes(), f
    base_cols = list(pd.read_csv(plain / "all_droplets.csv").columns)
    assert list(pd.read_csv(cells / "all_droplets.csv").columns) == base_cols + NEW_DROPLET_COLUMNS
    assert list(pd.read_csv(nuclei / "all_droplets.csv").columns) == base_cols + NEW_DROPLET_COLUMNS + ["nucleus_gap_px", "nucleus_gap_um"]
    base_sum = list(pd.read_csv(plain / "summary_per_image.csv").columns)
    for out in (cells, nuclei):
        assert list(pd.read_csv(out / "summary_per_image.csv").columns) == base_sum + SUMMARY_COLUMNS
        assert list(pd.read_csv(out / "cells_per_image.csv").columns) == ["filename"] + SUMMARY_COLUMNS
        assert pd.read_csv(out / "all_droplets.csv")[base_cols].equals(pd.read_csv(plain / "all_droplets.csv"))
    table = pd.read_csv(nuclei / "cells.csv")
    assert list(table.columns) == ["filename", "cell", "area_px", "area_um2", "touches_border", "n_droplets", "droplet_area_px",
                                   "droplet_area_frac", "droplet_mean_area_px", "droplet_std_area_px", "droplet_median_area_px",
                                   "droplet_max_area_px", "nucleus_area_px"]
    assert len(table) == 6 and table["cell"].tolist() == [1, 2, 3, 1, 2, 3] and len(pd.read_csv(cells / "cells.csv")) == 6
    assert "nucleus_area_px" not in pd.read_csv(cells / "cells.csv").columns
    # the territories round-trip: the PNG is the nearest-label transform of the nuclei as the script labels them, cut at 20 pixels
    for i, (h, w) in enumerate(SIZES):
        png = np.array(Image.open(nuclei / "cell_territories" / f"im{i}_cells.png"))
        nuc = ndimage.label(labelled[i] > 0)[0]
        want, d2 = ref.nearest_brute(nuc, 3, 20)
        assert png.shape == (h, w) and np.array_equal(png, want) and (want == 0).any()
        rows = table[table["filename"] == f"im{i}.png"]
        assert rows["area_px"].tolist() == [int((want == k).sum()) for k in (1, 2, 3)]
        assert rows["nucleus_area_px"].tolist() == [int((nuc == k).sum()) for k in (1, 2, 3)]
    # the droplet columns against the oracle on the files the run wrote
    d0 = pd.read_csv(cells / "im0_droplets.csv")
    lab = ndimage.label(np.array(Image.open(cells / "predicted_masks" / "im0_pred.png")) > 0)[0]
    out_d, out_c, _ = ref.cell_table_brute(lab, len(d0), labelled[0], 3)
    assert d0["cell"].tolist() == out_d[0].tolist() and d0["n_cells"].tolist() == out_d[2].tolist()
    assert np.allclose(d0["cell_overlap_frac"], out_d[1] / out_d[4]) and d0["outside_cells"].tolist() == (out_d[0] == 0).tolist()
    s = pd.read_csv(cells / "cells_per_image.csv")
    assert s["n_cells"].tolist() == [3, 3] and s["n_droplets_outside_cells"][0] == int((out_d[0] == 0).sum())


def test_sparse_label_ids_are_renumbered_for_the_buffers_and_reported_as_in_the_file(tmp_path, monkeypatch):
    """A 16-bit label image whose ids have gaps (3 -> 60000): the per-cell buffers are sized by the three cells there are, the
    tables carry the file's numbers, and everything else equals the run on the dense numbering."""
    import quantify_droplets_batch as q
    dense = write_masks(tmp_path / "dense", as_labels=True)
    (tmp_path / "sparse").mkdir()
    for i, m in enumerate(dense):
        Image.fromarray(np.where(m == 3, 60000, m).astype(np.uint16)).save(tmp_path / "sparse" / f"im{i}.png")
    lab, ids = q.decode_cells(tmp_path / "sparse" / "im0.png", True, 1)
    assert ids.tolist() == [1, 2, 60000] and int(lab.max()) == 3 and np.array_equal(lab, dense[0])
    assert q.decode_cells(tmp_path / "dense" / "im0.png", True, 1)[1] is None
    a = run(tmp_path, monkeypatch, "a", ["--cell_dir", str(tmp_path / "dense"), "--cell_labels"])
    b = run(tmp_path, monkeypatch, "b", ["--cell_dir", str(tmp_path / "sparse"), "--cell_labels"])
    for f in ("cells.csv", "all_droplets.csv"):
        ta, tb = pd.read_csv(a / f), pd.read_csv(b / f)
        assert tb["cell"].replace(60000, 3).tolist() == ta["cell"].tolist() and ta.drop(columns="cell").equals(tb.drop(columns="cell"))
    assert set(pd.read_csv(b / "cells.csv")["cell"]) == {1, 2, 60000}
    assert (a / "cells_per_image.csv").read_bytes() == (b / "cells_per_image.csv").read_bytes()


def test_cli_composes_with_split_touching(tmp_path, monkeypatch):
    write_masks(tmp_path / "nuc")
    out = run(tmp_path, monkeypatch, "split", ["--nuclei_dir", str(tmp_path / "nuc"), "--split_touching"])
    t = pd.read_csv(out / "im0_droplets.csv")
    assert len(t) == 2 and set(NEW_DROPLET_COLUMNS) <= set(t.columns)                 # the two discs, cut at the neck
    lab = np.array(Image.open(out / "predicted_masks" / "im0_labels.png"))
    terr = np.array(Image.open(out / "cell_territories" / "im0_cells.png"))
    assert t["cell"].tolist() == ref.cell_table_brute(lab, 2, terr, 3)[0][0].tolist()


def test_cli_composes_with_tile_and_tta(tmp_path, monkeypatch):
    """--tile with --tta: the network itself, one native-size map per image, the stage on batches of one."""
    import quantify_droplets_batch as q
    from scipy import ndimage
    from tests.test_tiling_cpu import SIZES as TILE_SIZES, calibrated_checkpoint, write_images
    monkeypatch.setattr(q, "DEVICE", "cpu")
    img_dir = tmp_path / "tile_imgs"
    write_images(img_dir)
    write_masks(tmp_path / "tile_nuc", TILE_SIZES)
    ck, _ = calibrated_checkpoint(tmp_path, img_dir, 15, 64, 16, 0.3, gain=4.0)
    out = q.main(["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--batch", "4", "--prob_thresh", "0.3", "--skip_excel",
                  "--skip_histogram", "--background_radius", "15", "--tile", "64", "--tile_overlap", "16", "--tta", "2",
                  "--out_dir", str(tmp_path / "tile"), "--nuclei_dir", str(tmp_path / "tile_nuc")])
    assert len(pd.read_csv(out / "cells_per_image.csv")) == 2 and len(pd.read_csv(out / "cells.csv")) == 6
    for i in range(2):
        t = pd.read_csv(out / f"im{i}_droplets.csv")
        lab = ndimage.label(np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0)[0]
        terr = np.array(Image.open(out / "cell_territories" / f"im{i}_cells.png"))
        assert terr.shape == TILE_SIZES[i] and len(t) == lab.max() > 0
        assert t["cell"].tolist() == ref.cell_table_brute(lab, len(t), terr, 3)[0][0].tolist()


def test_cli_argument_errors(tmp_path, monkeypatch, capsys):
    import quantify_droplets_batch as q
    write_masks(tmp_path / "nuc")
    base = ["--img_dir", str(tmp_path / "none"), "--out_dir", str(tmp_path / "out")]
    for extra, word in ((["--cell_dir", "a", "--nuclei_dir", "b"], "give one"), (["--cell_radius", "5"], "--nuclei_dir"),
                        (["--cell_dir", "a", "--cell_radius", "5"], "--nuclei_dir"), (["--cell_labels"], "needs one"),
                        (["--nuclei_dir", "b", "--cell_radius", "-1"], "0..32767")):
        with pytest.raises(SystemExit) as e:
            q.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    assert not (tmp_path / "out").exists()
    # a mask of another size than its image: an error that names the file, before anything runs
    (tmp_path / "bad").mkdir()
    for i in range(2):
        Image.fromarray(np.zeros((10, 10), np.uint8)).save(tmp_path / "bad" / f"im{i}.png")
    with pytest.raises(SystemExit) as e:
        run(tmp_path, monkeypatch, "bad_out", ["--nuclei_dir", str(tmp_path / "bad")])
    assert "--nuclei_dir" in str(e.value) and "im0.png" in str(e.value) and not (tmp_path / "bad_out").exists()
    (tmp_path / "bad" / "im1.png").unlink()
    Image.fromarray(np.zeros(SIZES[0], np.uint8)).save(tmp_path / "bad" / "im0.png")
    with pytest.raises(SystemExit) as e:
        run(tmp_path, monkeypatch, "bad_out", ["--cell_dir", str(tmp_path / "bad")])
    assert "--cell_dir" in str(e.value) and "im1.png" in str(e.value)


def test_wrapper_on_cpu_tensors_and_option_checks():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.cells import nearest_label
    from unet_dc_segmentation_amd.droplets import DropletOptions, _options
    label, max_label = ref.nearest_cases()["random_seeds"]
    lab, d2 = nearest_label(torch.from_numpy(label), max_label, 3)
    want = ref.nearest_brute(label, max_label, 3)
    assert np.array_equal(lab.numpy(), want[0]) and np.array_equal(d2.numpy(), want[1])
    with pytest.raises(_lib.UnetdcError):
        nearest_label(torch.from_numpy(label), max_label, -1)
    with pytest.raises(_lib.UnetdcError):
        nearest_label(torch.from_numpy(label).float(), max_label)
    assert not DropletOptions().cells and not DropletOptions().label_map and DropletOptions(cells=True).label_map
    with pytest.raises(_lib.UnetdcError):
        _options({"options": DropletOptions(cells=True)}, 0.5)                           # the field without the maps
    assert _options({"cells": ["maps"]}, 0.5)[0].cells
