"""CPU: the host path of the droplet split (utils/droplet_split.py) against the slow restatement of the same definition
(tests/split_ref.py), the properties the definition promises, the argument checks of the new C-ABI entry points, and
quantify_droplets_batch.py --split_touching on its CPU path."""
import math

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image
from scipy import ndimage

from tests.split_ref import edt_sq_ref, split_ref
from utils import droplet_split as ds


def noise_mask(h, w, seed, sigma=3.0, frac=0.5):
    """Thresholded smoothed noise: ragged blobs with necks of every width, some touching the border."""
    f = ndimage.gaussian_filter(np.random.default_rng(seed).random((h, w)), sigma)
    return (f > np.quantile(f, 1.0 - frac)).astype(np.uint8)


def small_masks():
    rng = np.random.default_rng(11)
    one = np.zeros((9, 7), np.uint8)
    one[4, 3] = 1
    return {"empty": np.zeros((12, 17), np.uint8), "full": np.ones((12, 17), np.uint8), "single": one,
            "1xN": (rng.random((1, 61)) < 0.7).astype(np.uint8), "Nx1": (rng.random((61, 1)) < 0.7).astype(np.uint8),
            "1x1_fg": np.ones((1, 1), np.uint8), "1x1_bg": np.zeros((1, 1), np.uint8)}


def host_rows(mask, h2, min_area=1):
    lab, a, sy, sx, first = ds.split_labels(mask, h2, min_area)
    return lab, [tuple(int(v) for v in r) for r in zip(a, sy, sx, first)]


def assert_equals_restatement(mask, h2, min_area=1):
    lab, rows = host_rows(mask, h2, min_area)
    rlab, rrows = split_ref(mask, h2, min_area)
    assert lab.dtype == np.int32 and np.array_equal(lab, rlab)
    assert rows == rrows


@pytest.mark.parametrize("shape,h2s", [((37, 53), (0, 1, 4, 7)), ((276, 408), (0, 1, 4, 7)), ((512, 512), (1, 4))])
def test_host_path_equals_restatement_on_noise(shape, h2s):
    m = noise_mask(*shape, seed=shape[0])
    assert np.array_equal(ds.edt_sq(m), edt_sq_ref(m))
    for h2 in h2s:
        assert_equals_restatement(m, h2)
    assert_equals_restatement(m, 4, min_area=30)


@pytest.mark.parametrize("name", sorted(small_masks()))
def test_host_path_equals_restatement_on_small_masks(name):
    m = small_masks()[name]
    assert np.array_equal(ds.edt_sq(m), edt_sq_ref(m))
    for h2 in (0, 1, 4, 7, 1000):
        assert_equals_restatement(m, h2)


def test_mask_without_background_is_one_droplet_at_infinite_distance():
    m = np.ones((12, 17), np.uint8)
    assert ds.EDT_INF == 2 ** 31 - 1 and np.all(ds.edt_sq(m) == ds.EDT_INF)
    for h2 in (0, 4):
        lab, rows = host_rows(m, h2)
        assert np.all(lab == 1) and rows == [(12 * 17, 17 * sum(range(12)), 12 * sum(range(17)), 0)]


def test_edt_ignores_the_outside_of_the_image():
    m = np.ones((5, 9), np.uint8)
    m[2, 0] = 0
    yy, xx = np.mgrid[0:5, 0:9]
    assert np.array_equal(ds.edt_sq(m), (yy - 2) ** 2 + xx ** 2)


def scipy_table(mask, min_area):
    lbl, n = ndimage.label(mask)
    rows = []
    for k in range(1, n + 1):
        ys, xs = np.nonzero(lbl == k)
        if len(ys) >= max(min_area, 1):
            rows.append((len(ys), int(ys.sum()), int(xs.sum()), int(ys[0] * mask.shape[1] + xs[0])))
    return lbl, rows


@pytest.mark.parametrize("shape", [(37, 53), (150, 200), (1, 61), (61, 1)])
@pytest.mark.parametrize("min_area", [1, 12])
def test_large_depth_equals_connected_components(shape, min_area):
    m = noise_mask(*shape, seed=3, sigma=1.5 if min(shape) > 1 else 0.0, frac=0.45)
    h2 = 2 * math.ceil(math.hypot(*shape))
    lab, rows = host_rows(m, h2, min_area)
    lbl, ref = scipy_table(m, min_area)
    assert rows == ref and (min_area > 1 or len(ref) > 1)
    if min_area == 1:
        assert np.array_equal(lab, lbl)
    assert host_rows(m, 10 ** 9, min_area)[1] == ref         # any larger depth: the same


@pytest.mark.parametrize("h2", [0, 1, 4, 7])
def test_no_droplet_spans_two_components(h2):
    m = noise_mask(150, 200, seed=5)
    lab, rows = host_rows(m, h2)
    lbl, n = ndimage.label(m)
    assert np.array_equal(lab > 0, m > 0)
    pairs = np.unique(np.stack([lab[m > 0], lbl[m > 0]], 1), axis=0)
    assert len(pairs) == len(rows) and len(np.unique(pairs[:, 0])) == len(rows)     # one component per droplet
    assert len(rows) >= n
    # every droplet is itself 4-connected
    for k in range(1, len(rows) + 1, max(1, len(rows) // 25)):
        assert ndimage.label(lab == k)[1] == 1


def two_discs(r, d, oy, ox):
    """Two discs of radius r, centres d apart along x, the first centre at a sub-pixel offset (oy, ox)."""
    pad = 4
    h, w = int(2 * r + 2 * pad + 2), int(2 * r + d + 2 * pad + 2)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = r + pad + oy, r + pad + ox
    return (((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) | ((yy - cy) ** 2 + (xx - cx - d) ** 2 <= r * r)).astype(np.uint8)


def test_disc_pairs_split_by_the_depth_of_their_neck():
    """Two equal discs of radius r at centre distance d have a neck of half width sqrt(r^2 - d^2 / 4): the distance transform
    dips r - sqrt(r^2 - d^2 / 4) below its two peaks.  2 droplets where that depth is >= H2 / 2 + 1.5 px, 1 where it is
    <= H2 / 2 - 1.5 px (the pixel grid moves it by under a pixel); the cases in between are counted, not asserted."""
    h2 = 4
    cases = [(r, f) for r in (6, 12, 20, 40) for f in (0.25, 0.5, 1.0, 1.3, 1.5, 1.7, 1.9)]
    unasserted = 0
    for r, f in cases:
        d = f * r
        depth = r - math.sqrt(r * r - d * d / 4)
        expect = 2 if depth >= h2 / 2 + 1.5 else 1 if depth <= h2 / 2 - 1.5 else None
        if expect is None:
            unasserted += 1
            continue
        for oy, ox in ((0.0, 0.0), (0.5, 0.25), (0.3, 0.7)):
            n = len(host_rows(two_discs(r, d, oy, ox), h2)[1])
            assert n == expect, (r, f, oy, ox, depth, n)
    assert len(cases) == 28 and unasserted == 9 and unasserted <= 0.4 * len(cases)


@pytest.mark.parametrize("axes", [(50, 12), (60, 12), (40, 16), (80, 16), (30, 30)])
def test_ellipses_stay_whole_at_the_default_depth(axes):
    """An ellipse's inscribed-circle radius falls monotonically from the centre to the tips, so its distance transform has one
    peak; the pixel grid breaks it into many basins whose saddles lie a fraction of a pixel deep -- far less than 2 px."""
    a, b = axes[0] / 2, axes[1] / 2
    yy, xx = np.mgrid[0:100, 0:100]
    for ang in (0, 30, 45, 90):
        c, s = math.cos(math.radians(ang)), math.sin(math.radians(ang))
        u, v = (xx - 49.3) * c + (yy - 50.6) * s, -(xx - 49.3) * s + (yy - 50.6) * c
        m = ((u / a) ** 2 + (v / b) ** 2 <= 1).astype(np.uint8)
        assert len(host_rows(m, 4)[1]) == 1, (axes, ang)


def test_small_disc_on_the_rim_of_a_large_one_is_split():
    yy, xx = np.mgrid[0:80, 0:90]
    m = (((yy - 40) ** 2 + (xx - 35) ** 2 <= 400) | ((yy - 40) ** 2 + (xx - 60) ** 2 <= 81)).astype(np.uint8)
    lab, rows = host_rows(m, 4)
    assert len(rows) == 2 and ndimage.label(m)[1] == 1


def test_half_pixels():
    assert [ds.half_pixels(v) for v in (0, 0.5, 2, 2.0, 3.5)] == [0, 1, 4, 4, 7]
    for bad in (-0.5, 0.3, 2.25, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ds.half_pixels(bad)


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_split_abi_rejects_bad_arguments(lib):
    import ctypes
    from unet_dc_segmentation_amd import _lib
    assert _lib.EDT_INF == ds.EDT_INF
    n = 1040 * 1388
    assert lib.unetdc_split_workspace(1040, 1388) >= lib.unetdc_ccl_workspace(1040, 1388) + 8 * n
    assert lib.unetdc_split_workspace(0, 1388) == 0
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every check below fails before any HIP call

    def split(h=64, w=64, depth=4, mask=fake, bytes_=1 << 30, max_out=10):
        return lib.unetdc_split_stats(mask, h, w, 1, depth, fake, bytes_, fake, fake, fake, fake, None, None, max_out, None)
    for kw, msg in [(dict(mask=None), b"null"), (dict(h=0), b"geometry"), (dict(w=16385), b"geometry"),
                    (dict(max_out=-1), b"geometry"), (dict(depth=-1), b"depth")]:
        assert split(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    assert split(bytes_=lib.unetdc_split_workspace(64, 64) - 1) == -3 and b"workspace" in lib.unetdc_last_error()
    assert lib.unetdc_edt_sq(None, 64, 64, fake, fake, 1 << 30, None) == -1 and b"null" in lib.unetdc_last_error()
    assert lib.unetdc_edt_sq(fake, 64, 0, fake, fake, 1 << 30, None) == -1 and b"geometry" in lib.unetdc_last_error()
    assert lib.unetdc_edt_sq(fake, 64, 64, fake, fake, 4 * 64 * 64, None) == -3 and b"workspace" in lib.unetdc_last_error()


# ---- quantify_droplets_batch.py on the CPU path --------------------------------------------------------------------------
SIZE = 64


class FixedProbs(torch.nn.Module):
    """Stands in for the network: the k-th image of the run gets the k-th of the given probability maps."""

    def __init__(self, probs):
        super().__init__()
        self.probs, self.k = probs, 0

    def forward(self, batch):
        out = self.probs[self.k:self.k + len(batch)].to(batch.device)
        self.k += len(batch)
        return out


def cli_probs():
    """Three 64 x 64 maps: two overlapping discs, smooth noise, nothing."""
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    discs = ((yy - 32) ** 2 + (xx - 20) ** 2 <= 144) | ((yy - 32) ** 2 + (xx - 41) ** 2 <= 144)
    p = np.stack([np.where(discs, 0.9, 0.1), np.where(noise_mask(SIZE, SIZE, 2) > 0, 0.8, 0.2), np.full((SIZE, SIZE), 0.1)])
    return torch.from_numpy(p.astype(np.float32))[:, None]


def run_cli(tmp_path, monkeypatch, tag, extra, device="cpu", sizes=((SIZE, SIZE),) * 3, probs=None):
    import quantify_droplets_batch as q
    monkeypatch.setattr(q, "DEVICE", device)
    monkeypatch.setattr(q, "IMG_SIZE", SIZE if probs is None else probs.shape[-1])
    probs = cli_probs() if probs is None else probs
    monkeypatch.setattr(q, "load_model", lambda ckpt, dtype="f32": FixedProbs(probs))
    img_dir = tmp_path / "imgs"
    if not img_dir.exists():
        img_dir.mkdir()
        rng = np.random.default_rng(0)
        for i, (h, w) in enumerate(sizes):
            Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(img_dir / f"im{i}.png")
    return q.main(["--img_dir", str(img_dir), "--out_dir", str(tmp_path / tag), "--batch", "2", "--skip_excel",
                   "--skip_histogram", "--background_radius", "15", "--prob_thresh", "0.5", *extra])


def files(d):
    return sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file())


def test_cli_without_the_flag_is_the_connected_component_flow(tmp_path, monkeypatch):
    import quantify_droplets_batch as q
    plain = run_cli(tmp_path, monkeypatch, "plain", ["--save_overlays"])
    assert not any("labels" in f for f in files(plain))
    masks = [(cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8) for i in range(3)]
    for i, m in enumerate(masks):
        assert np.array_equal(np.array(Image.open(plain / "predicted_masks" / f"im{i}_pred.png")), m * 255)
        ref = q.quantify(m, 1, None)                     # scipy's label: the flow as it was
        if ref.empty:
            continue
        got = pd.read_csv(plain / f"im{i}_droplets.csv", float_precision="round_trip")
        assert np.array_equal(got["area"].to_numpy(), ref["area"].to_numpy())
        assert np.array_equal(got["centroid-0"].to_numpy(), ref["centroid-0"].to_numpy())
    summary = pd.read_csv(plain / "summary_per_image.csv")
    assert summary["droplet_count"].tolist() == [ndimage.label(m)[1] for m in masks] and summary["droplet_count"][0] == 1
    # a depth at which nothing is cut: every file of the plain run again, byte for byte, plus the label images
    deep = run_cli(tmp_path, monkeypatch, "deep", ["--save_overlays", "--split_touching", "--split_depth", "1000"])
    assert sorted(set(files(deep)) - set(files(plain))) == [f"predicted_masks/im{i}_labels.png" for i in range(3)]
    for f in files(plain):
        assert (plain / f).read_bytes() == (deep / f).read_bytes(), f


def test_cli_split_touching_on_the_cpu_path(tmp_path, monkeypatch):
    plain = run_cli(tmp_path, monkeypatch, "plain", ["--save_overlays"])
    out = run_cli(tmp_path, monkeypatch, "split", ["--split_touching", "--save_overlays", "--density_maps"])
    dens = run_cli(tmp_path, monkeypatch, "dens", ["--density_maps"])
    t0 = pd.read_csv(out / "im0_droplets.csv")
    assert len(t0) == 2 and t0["label"].tolist() == [1, 2]                    # the two discs, cut at the neck
    assert abs(t0["centroid-1"][0] - 20) < 1.5 and abs(t0["centroid-1"][1] - 41) < 1.5
    summary = pd.read_csv(out / "summary_per_image.csv")
    assert summary["droplet_count"].tolist()[0] == 2 and summary["droplet_count"][2] == 0
    assert summary["total_area_px"].tolist() == pd.read_csv(plain / "summary_per_image.csv")["total_area_px"].tolist()
    all_d = pd.read_csv(out / "all_droplets.csv")
    assert len(all_d) == summary["droplet_count"].sum()
    for i in range(3):
        png = Image.open(out / "predicted_masks" / f"im{i}_labels.png")
        lab = np.array(png)
        assert png.mode in ("I;16", "I;16B", "I") and lab.shape == (SIZE, SIZE)
        m = (cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8)
        ref_lab, rows = split_ref(m, 4)
        assert np.array_equal(lab, ref_lab) and summary["droplet_count"][i] == len(rows)
        assert (out / "predicted_masks" / f"im{i}_pred.png").read_bytes() == (plain / "predicted_masks" / f"im{i}_pred.png").read_bytes()
    # the overlay shows the cut: the pixels on both sides of the neck are painted
    ov, ov0 = (np.array(Image.open(d / "overlays" / "im0_overlay.png")) for d in (out, plain))
    changed = np.any(ov != ov0, axis=-1)
    lab0 = np.array(Image.open(out / "predicted_masks" / "im0_labels.png"))
    assert changed.any() and np.all(ds.label_boundaries(lab0)[changed])
    # the density maps keep counting connected components
    for f in ["density_per_image.csv"] + [f"im{i}_{k}_density.png" for i in range(3) for k in ("radial", "spatial")]:
        assert (out / f).read_bytes() == (dens / f).read_bytes(), f


@pytest.mark.parametrize("bad", ["-1", "0.3", "2.25", "nan"])
def test_cli_refuses_a_bad_split_depth_before_any_image(tmp_path, monkeypatch, bad):
    with pytest.raises(SystemExit):
        run_cli(tmp_path, monkeypatch, "bad", ["--split_touching", "--split_depth", bad])
    assert not (tmp_path / "bad").exists()
