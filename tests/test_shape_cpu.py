"""CPU: the host path of the per-droplet shape and intensity table (utils/droplet_shape.py) against
the plain-loop restatement (tests/shape_ref.py), an independent scipy route for the perimeter, known answers and closed
forms of the derived columns, the argument checks of the two new C-ABI entry points, and
quantify_droplets_batch.py --droplet_shape on its CPU path."""
import math

import numpy as np
import pandas as pd
import pytest
from scipy import ndimage

from tests.shape_ref import label_props_ref
from tests.test_split_cpu import cli_probs, files, noise_mask, run_cli, small_masks
from utils import droplet_shape as sh
from utils import droplet_split as ds


def cc_labels(mask, min_area=1):
    """scipy's 4-connected labelling, objects below min_area dropped, renumbered in raster order of the first pixel."""
    lbl, n = ndimage.label(mask)
    if n:
        keep = np.bincount(lbl.ravel(), minlength=n + 1) >= max(min_area, 1)
        keep[0] = False
        lbl = ndimage.label(keep[lbl])[0]
    return lbl.astype(np.int32)


def split_labels(mask, h2=4, min_area=1):
    return ds.split_labels(mask, h2, min_area)[0]


def gray_plane(h, w, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def label_inputs():
    """name -> int32 label map: the small masks and noise masks of test_split_cpu, labelled as connected components and as
    split droplets at depth 2.0 (labels that touch each other), full foreground, a checkerboard, a 1 x N and an N x 1 image."""
    masks = dict(small_masks())
    masks["noise37x53"] = noise_mask(37, 53, seed=37)
    masks["noise90x120"] = noise_mask(90, 120, seed=5)
    out = {}
    for name, m in masks.items():
        out[name + "/cc"] = cc_labels(m)
        out[name + "/split"] = split_labels(m)
    yy, xx = np.mgrid[0:21, 0:30]
    out["checkerboard"] = cc_labels(((yy + xx) % 2).astype(np.uint8))
    out["full70x67"] = np.ones((70, 67), np.int32)
    return out


INPUTS = label_inputs()


def assert_equals_restatement(labels, gray):
    got = sh.label_props_numpy(labels, gray)
    ref = label_props_ref(labels.tolist(), None if gray is None else gray.tolist())
    k = int(labels.max(initial=0))
    assert sorted(ref) == list(range(1, k + 1))
    names = ("area", "Sy", "Sx") + (sh.QUANTITIES if gray is not None else sh.QUANTITIES[:10])
    assert sorted(got) == sorted(names)
    for q in names:
        assert got[q].dtype == np.int64 and got[q].shape == (k,)
        assert got[q].tolist() == [ref[i][q] for i in range(1, k + 1)], q


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_numpy_path_equals_plain_loops(name):
    lab = INPUTS[name]
    assert_equals_restatement(lab, gray_plane(*lab.shape))
    assert_equals_restatement(lab, None)


def test_inputs_hold_touching_labels_and_single_pixels():
    assert ds.label_boundaries(INPUTS["noise90x120/split"]).any()
    assert sh.label_props_numpy(INPUTS["checkerboard"])["area"].tolist() == [1] * 315
    assert INPUTS["1xN/cc"].shape == (1, 61) and INPUTS["Nx1/cc"].shape == (61, 1)


def perimeter_scipy(labels):
    """The independent route: per label on its own binary image, erosion with the cross (outside = background), the
    weighted 3 x 3 convolution of the border image, and a histogram of the codes."""
    w = np.zeros(50)
    w[[5, 7, 15, 17, 25, 27]] = 1
    w[[21, 33]] = math.sqrt(2)
    w[[13, 23]] = (1 + math.sqrt(2)) / 2
    out = []
    for k in range(1, int(labels.max(initial=0)) + 1):
        img = (labels == k).astype(np.uint8)
        border = img - ndimage.binary_erosion(img, ndimage.generate_binary_structure(2, 1), border_value=0)
        codes = ndimage.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
        out.append(np.bincount(codes.ravel(), minlength=50)[:50] @ w)
    return np.array(out)


def columns(labels, gray=None, px=None):
    return sh.shape_columns(sh.label_props_numpy(labels, gray), labels.shape, px)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_perimeter_equals_scipy_route(name):
    lab = INPUTS[name]
    got = columns(lab)["perimeter"]
    ref = perimeter_scipy(lab)
    assert got.shape == ref.shape and np.allclose(got, ref, rtol=1e-12, atol=0)


def rect(a, b, pad=3):
    m = np.zeros((a + 2 * pad, b + 2 * pad), np.int32)
    m[pad:pad + a, pad:pad + b] = 1
    return m


@pytest.mark.parametrize("a,b,perimeter", [(1, 1, 0), (2, 2, 4), (3, 3, 8), (1, 3, 1), (5, 7, 20)])
def test_known_perimeters_of_rectangles(a, b, perimeter):
    c = columns(rect(a, b))
    assert c["perimeter"].tolist() == [perimeter]
    assert c["circularity"][0] == (0.0 if perimeter == 0 else 4 * math.pi * a * b / perimeter ** 2)


def test_known_answer_of_the_disc():
    yy, xx = np.mgrid[0:101, 0:101]
    disc = ((yy - 50) ** 2 + (xx - 50) ** 2 <= 40 ** 2).astype(np.int32)
    p = sh.label_props_numpy(disc)
    c = sh.shape_columns(p, disc.shape)
    assert p["area"].tolist() == [5025]
    assert abs(c["perimeter"][0] - 263.7645019878171) <= 1e-12 * 263.7645019878171
    assert abs(c["circularity"][0] - 0.90763918) < 1e-8
    assert c["eccentricity"][0] == 0.0 and c["orientation"][0] == -math.pi / 4 and not c["touches_border"][0]
    assert abs(c["axis_major_length"][0] - 80.0) < 0.5 and c["axis_major_length"][0] == c["axis_minor_length"][0]


@pytest.mark.parametrize("a,b", [(5, 7), (7, 5), (2, 9), (4, 4), (1, 1), (1, 6), (6, 1)])
def test_closed_forms_of_a_filled_rectangle(a, b):
    """a rows x b columns: variances (a^2 - 1) / 12 and (b^2 - 1) / 12, no covariance."""
    c = columns(rect(a, b))
    big, small = max(a, b), min(a, b)
    assert np.isclose(c["axis_major_length"][0], 4 * math.sqrt((big * big - 1) / 12), rtol=1e-15)
    assert np.isclose(c["axis_minor_length"][0], 4 * math.sqrt((small * small - 1) / 12), rtol=1e-15)
    ecc = 0.0 if big == 1 else math.sqrt(1 - (small * small - 1) / (big * big - 1))
    assert np.isclose(c["eccentricity"][0], ecc, rtol=1e-15, atol=0)
    # taller than wide: 0; wider than tall: +pi / 2 (a zero covariance carries sign +); neither: -pi / 4
    assert c["orientation"][0] == (0.0 if a > b else math.pi / 2 if b > a else -math.pi / 4)
    assert [int(c[f"bbox-{i}"][0]) for i in range(4)] == [3, 3, 3 + a, 3 + b] and not c["touches_border"][0]


def test_five_by_seven_in_numbers():
    c = columns(rect(5, 7))
    assert np.isclose(c["axis_major_length"][0], 8.0, rtol=1e-15) and np.isclose(c["axis_minor_length"][0], 5.656854249492381, rtol=1e-15)
    assert np.isclose(c["eccentricity"][0], math.sqrt(0.5), rtol=1e-15)


def test_orientation_of_diagonal_lines():
    n = 9
    main = np.eye(n, dtype=np.int32)                       # y = x: positive covariance, equal variances
    anti = np.ascontiguousarray(main[:, ::-1])
    assert columns(main)["orientation"][0] == math.pi / 4
    assert columns(anti)["orientation"][0] == -math.pi / 4
    for lab in (main, anti):
        c = columns(lab)
        assert np.isclose(c["eccentricity"][0], 1.0, rtol=1e-15) and c["axis_minor_length"][0] < 1e-6
        assert c["perimeter"][0] == perimeter_scipy(lab)[0]


def test_bbox_and_touches_border_at_every_edge():
    h, w = 20, 30
    lab = np.zeros((h, w), np.int32)
    boxes = [(0, 5, 2, 8), (8, 0, 11, 3), (17, 12, 20, 15), (9, 27, 12, 30), (5, 10, 9, 14), (17, 0, 20, 2)]
    for k, (y0, x0, y1, x1) in enumerate(boxes, 1):
        lab[y0:y1, x0:x1] = k
    c = columns(lab)
    assert [tuple(int(c[f"bbox-{i}"][k]) for i in range(4)) for k in range(len(boxes))] == boxes
    assert c["touches_border"].tolist() == [True, True, True, True, False, True]     # top, left, bottom, right, inside, corner
    assert c["touches_border"].dtype == bool


def test_variance_numerators_are_exact_past_64_bits():
    """A droplet of 2^26 pixels whose rows run up to 16383: A * Syy ~ 2^26 * 2^54 passes 2^63.  Two droplets whose integers
    differ in the last place of Syy give variances that differ by exactly 1 / A in exact arithmetic; float64 products
    of A * Syy would round that away."""
    A = 2 ** 26
    Sy = A * 12000
    Syy = A * 12000 * 12000 + A * 9
    assert A * Syy > 2 ** 63
    props = {q: np.array([v, v], dtype=np.int64) for q, v in
             (("area", A), ("Sy", Sy), ("Sx", A * 100), ("Sxx", A * 100 * 100 + A * 4), ("Sxy", 12000 * 100 * A),
              ("min_y", 1), ("min_x", 1), ("max_y", 5), ("max_x", 5), ("P1", 4), ("P2", 0), ("P3", 0))}
    props["Syy"] = np.array([Syy, Syy + 2 ** 20], dtype=np.int64)
    c = sh.shape_columns(props, (16384, 16384))
    assert c["axis_major_length"][0] == 4 * math.sqrt(9.0) and c["axis_minor_length"][0] == 4 * math.sqrt(4.0)
    assert c["axis_major_length"][1] == 4 * math.sqrt(9.0 + 2.0 ** -6)        # (A * 2^20) / A^2, exactly representable
    assert float(A) * float(Syy + 1) == float(A) * float(Syy)                  # what float64 products would have lost
    assert c["orientation"].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("name", ["noise90x120/cc", "noise90x120/split", "checkerboard", "1xN/cc"])
def test_intensity_equals_ndimage(name):
    lab = INPUTS[name]
    g = gray_plane(*lab.shape, seed=4)
    idx = np.arange(1, int(lab.max()) + 1)
    p = sh.label_props_numpy(lab, g)
    g64 = g.astype(np.int64)
    assert np.array_equal(p["Sg"], np.rint(ndimage.sum(g64, lab, idx)).astype(np.int64))
    assert np.array_equal(p["Sgg"], np.rint(ndimage.sum(g64 * g64, lab, idx)).astype(np.int64))
    assert np.array_equal(p["min_g"], ndimage.minimum(g64, lab, idx)) and np.array_equal(p["max_g"], ndimage.maximum(g64, lab, idx))
    c = sh.shape_columns(p, lab.shape)
    assert np.allclose(c["intensity_mean"], ndimage.mean(g64, lab, idx), rtol=1e-13)
    assert np.allclose(c["intensity_std"], ndimage.standard_deviation(g64, lab, idx), rtol=1e-9, atol=1e-9)
    assert np.array_equal(c["intensity_min"], p["min_g"]) and np.array_equal(c["intensity_max"], p["max_g"])


def test_micron_columns():
    lab = INPUTS["noise37x53/cc"]
    c, cm = columns(lab), columns(lab, px=3.45)
    assert list(cm)[-3:] == ["perimeter_micron", "axis_major_micron", "axis_minor_micron"] and list(cm)[:-3] == list(c)
    assert np.array_equal(cm["perimeter_micron"], c["perimeter"] / 3.45)
    assert np.array_equal(cm["axis_major_micron"], c["axis_major_length"] / 3.45)


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_shape_abi_rejects_bad_arguments(lib):
    import ctypes
    n = 1040 * 1388
    assert lib.unetdc_ccl_labels_workspace(1040, 1388) >= lib.unetdc_ccl_workspace(1040, 1388) + 4 * n
    assert lib.unetdc_ccl_labels_workspace(0, 1388) == 0
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every check below fails before any HIP call

    def labels(h=64, w=64, mask=fake, label=fake, bytes_=1 << 30, max_out=10):
        return lib.unetdc_ccl_labels(mask, h, w, 1, fake, bytes_, fake, fake, fake, fake, None, label, max_out, None)
    for kw, msg in [(dict(mask=None), b"null"), (dict(label=None), b"null"), (dict(h=0), b"geometry"), (dict(max_out=-1), b"geometry")]:
        assert labels(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    assert labels(bytes_=lib.unetdc_ccl_labels_workspace(64, 64) - 1) == -3 and b"workspace" in lib.unetdc_last_error()

    def props(label=fake, h=64, w=64, out=fake, max_out=10):
        return lib.unetdc_label_props(label, None, h, w, out, max_out, None)
    for kw, msg in [(dict(label=None), b"null"), (dict(out=None), b"null"), (dict(w=0), b"geometry"), (dict(h=16385), b"geometry"),
                    (dict(max_out=-1), b"geometry")]:
        assert props(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    assert lib.unetdc_version() == 2


# ---- quantify_droplets_batch.py --droplet_shape on the CPU path ----------------------------------------------------------
BASE_COLUMNS = ["filename", "label", "area", "equivalent_diameter", "centroid-0", "centroid-1"]
SHAPE_COLUMNS = ["perimeter", "circularity", "axis_major_length", "axis_minor_length", "eccentricity", "orientation", "bbox-0",
                 "bbox-1", "bbox-2", "bbox-3", "touches_border", "intensity_mean", "intensity_min", "intensity_max", "intensity_std"]


def cli_gray(tmp_path, i):
    from PIL import Image
    from utils.density import rgb_to_gray
    return rgb_to_gray(np.array(Image.open(tmp_path / "imgs" / f"im{i}.png").convert("RGB")))


@pytest.mark.parametrize("split", [False, True])
def test_cli_droplet_shape_on_the_cpu_path(tmp_path, monkeypatch, split):
    extra = ["--split_touching"] if split else []
    plain = run_cli(tmp_path, monkeypatch, "plain", extra + ["--density_maps"])
    out = run_cli(tmp_path, monkeypatch, "shape", extra + ["--density_maps", "--droplet_shape"])
    assert files(out) == files(plain)
    tables = {"all_droplets.csv"} | {f"im{i}_droplets.csv" for i in range(3)}
    for f in files(plain):                                   # everything but the droplet tables: byte for byte
        if f not in tables:
            assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    all_rows = []
    for i in range(3):
        m = (cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8)
        lab = split_labels(m) if split else cc_labels(m)
        if lab.max() == 0:
            assert (out / f"im{i}_droplets.csv").read_bytes() == (plain / f"im{i}_droplets.csv").read_bytes()
            continue
        got = pd.read_csv(out / f"im{i}_droplets.csv", float_precision="round_trip")
        old = pd.read_csv(plain / f"im{i}_droplets.csv", float_precision="round_trip")
        assert list(got.columns) == BASE_COLUMNS + SHAPE_COLUMNS and list(old.columns) == BASE_COLUMNS
        assert got[BASE_COLUMNS[:4]].equals(old[BASE_COLUMNS[:4]])
        assert np.allclose(got["centroid-0"], old["centroid-0"], rtol=1e-14) and np.allclose(got["centroid-1"], old["centroid-1"], rtol=1e-14)
        ref = sh.shape_columns(sh.label_props_numpy(lab, cli_gray(tmp_path, i)), lab.shape)
        assert len(got) == lab.max()
        for name in SHAPE_COLUMNS:
            assert np.array_equal(got[name].to_numpy(), ref[name]), name
        all_rows.append(got)
    combined = pd.read_csv(out / "all_droplets.csv", float_precision="round_trip")
    assert combined.equals(pd.concat(all_rows, ignore_index=True))
    if split:                                                # the two discs of image 0, cut: each rounder than the pair
        whole = pd.read_csv(run_cli(tmp_path, monkeypatch, "whole", ["--droplet_shape"]) / "im0_droplets.csv")
        cut = pd.read_csv(out / "im0_droplets.csv")
        assert len(whole) == 1 and len(cut) == 2 and cut["circularity"].min() > whole["circularity"][0]


def test_cli_micron_columns_and_flag_off_is_unchanged(tmp_path, monkeypatch):
    a = run_cli(tmp_path, monkeypatch, "a", ["--px_per_micron", "3.45"])
    b = run_cli(tmp_path, monkeypatch, "b", ["--px_per_micron", "3.45", "--droplet_shape"])
    ta, tb = pd.read_csv(a / "all_droplets.csv"), pd.read_csv(b / "all_droplets.csv")
    assert list(tb.columns) == list(ta.columns) + SHAPE_COLUMNS + ["perimeter_micron", "axis_major_micron", "axis_minor_micron"]
    assert np.allclose(tb["perimeter_micron"] * 3.45, tb["perimeter"], rtol=1e-15)
    for f in ("summary_per_image.csv", "droplet_size_stats.csv"):
        assert (a / f).read_bytes() == (b / f).read_bytes()
