"""CPU: the host restatement of the density-map analysis (utils/density.py) against literal transcriptions of OpenCV's and
the reference's definitions, the argument checks of the new C-ABI entry points, and quantify_droplets_batch.py
--density_maps on its CPU path."""
import os
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image
from scipy import ndimage

from utils import density as hd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cell_image(h, w, seed=0):
    """Synthetic "cell": a bright ellipse on a dark noisy background, with small bright droplets inside and outside it;
    returns (rgb uint8 [h, w, 3], droplet mask uint8 {0, 1})."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cell = ((yy - 0.45 * h) / (0.32 * h)) ** 2 + ((xx - 0.55 * w) / (0.3 * w)) ** 2 <= 1
    img = 30 + 110 * cell + rng.normal(0, 8, (h, w))
    mask = np.zeros((h, w), np.uint8)
    for _ in range(max(4, h * w // 4000)):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.uniform(1, 5)
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        mask[d] = 1
        img[d] += 60
    g = np.clip(img, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, (g * 0.8).astype(np.uint8), g // 2], -1)), mask


def test_blur_taps_are_opencvs_fixed_point_kernel():
    assert hd.BLUR_TAPS.tolist() == [1, 3, 6, 12, 20, 30, 36, 40, 36, 30, 20, 12, 6, 3, 1]
    assert hd.BLUR_TAPS.sum() == 256


@pytest.mark.parametrize("shape", [(2, 2), (3, 9), (8, 8), (21, 34)])
def test_blur_equals_brute_force_2d_sum(shape):
    g = np.random.default_rng(shape[0]).integers(0, 256, shape).astype(np.uint8)
    k = hd.BLUR_TAPS
    p = np.pad(g.astype(np.int64), 7, mode="reflect")
    ref = np.zeros(shape, np.int64)
    for i in range(15):
        for j in range(15):
            ref += int(k[i]) * int(k[j]) * p[i:i + shape[0], j:j + shape[1]]
    assert np.array_equal(hd.gaussian_blur_u8(g), ((ref + 32768) >> 16).astype(np.uint8))


def test_gray_is_cv2_fixed_point_rule():
    rgb = np.random.default_rng(0).integers(0, 256, (5, 7, 3)).astype(np.uint8)
    r, g, b = (rgb[..., c].astype(int) for c in range(3))
    assert np.array_equal(hd.rgb_to_gray(rgb), (4899 * r + 9617 * g + 1868 * b + 8192) >> 14)


def otsu_exact(hist):
    """argmax of the between-class variance in exact rational arithmetic, with OpenCV's skip rule, first maximum wins."""
    n = sum(int(v) for v in hist)
    p = [Fraction(int(v), n) for v in hist]
    mu = sum(i * p[i] for i in range(256))
    eps = Fraction(hd.FLT_EPSILON)
    best, arg, q1, s1 = Fraction(0), 0, Fraction(0), Fraction(0)
    for i in range(256):
        q1 += p[i]
        s1 += i * p[i]
        q2 = 1 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1 - eps:
            continue
        mu1, mu2 = s1 / q1, (mu - s1) / q2
        sb = q1 * q2 * (mu1 - mu2) ** 2
        if sb > best:
            best, arg = sb, i
    return arg


def test_otsu_matches_exact_argmax():
    rng = np.random.default_rng(3)
    hists = [rng.integers(0, 1000, 256) for _ in range(6)]
    hists.append(np.bincount(np.clip(np.concatenate([rng.normal(60, 10, 5000), rng.normal(170, 20, 3000)]), 0, 255)
                             .astype(int), minlength=256))
    for spec in ([(0, 7)], [(37, 100)], [(10, 5), (200, 5)], [(0, 1), (255, 1)], [(100, 3), (101, 3)], [(0, 50), (128, 50), (255, 50)]):
        h = np.zeros(256, np.int64)
        for b, c in spec:
            h[b] = c
        hists.append(h)
    for h in hists:
        assert hd.otsu_threshold(h) == otsu_exact(h), np.nonzero(h)


def stripe_image():
    """8 x 108 gray stripes 0 / 100 / 200 of widths 23 / 62 / 23 (as RGB): after the blur, two Otsu splits tie."""
    g = np.zeros((8, 108), np.uint8)
    g[:, 23:85] = 100
    g[:, 85:] = 200
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1))


def test_otsu_tie_needs_two_roundings_per_step():
    """On the stripe image the threshold hangs on the rounding of q1 += h_i * scale: OpenCV's two roundings (the restatement,
    and the kernel since its products are opaque) give the exact argmax 58, a fused multiply-add gives 128."""
    h = np.bincount(hd.gaussian_blur_u8(hd.rgb_to_gray(stripe_image())).ravel(), minlength=256)
    assert hd.otsu_threshold(h) == otsu_exact(h) == 58
    scale = 1.0 / h.sum()
    mu = sum(i * float(h[i]) for i in range(256)) * scale
    mu1 = q1 = best = 0.0
    arg = 0
    for i in range(256):
        p_i = h[i] * scale
        mu1 *= q1
        q1 = float(Fraction(int(h[i])) * Fraction(scale) + Fraction(q1))      # fma(h_i, scale, q1): one rounding
        q2 = 1.0 - q1
        if min(q1, q2) < hd.FLT_EPSILON or max(q1, q2) > 1.0 - hd.FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sb = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sb > best:
            best, arg = sb, i
    assert arg == 128


def test_morphology_equals_scipy_grey_morphology():
    a = (np.random.default_rng(4).random((50, 70)) < 0.4).astype(np.uint8) * 255
    for is_max in (True, False):
        got = hd.morph_rect(a, 15, is_max)
        ref = (ndimage.grey_dilation(a, size=(15, 15), mode="constant", cval=0) if is_max else
               ndimage.grey_erosion(a, size=(15, 15), mode="constant", cval=255))
        assert np.array_equal(got, ref)


def test_linspace_bounds_formula():
    """np.linspace(0, maxd, 11) == [i * (maxd / 10) for i < 10] + [maxd] for every maxd = sqrt(k), k <= 1040^2 + 1388^2.
    (k = 0 alone: with an array of endpoints numpy takes its zero-step branch for the whole array once one step is 0.)"""
    assert np.array_equal(np.linspace(0, 0.0, 11), hd.ring_bounds(0.0, 10))
    kmax = 1040 ** 2 + 1388 ** 2
    for lo in range(1, kmax + 1, 1 << 19):
        k = np.arange(lo, min(lo + (1 << 19), kmax + 1))
        maxd = np.sqrt(k.astype(np.float64))
        ref = np.linspace(0, maxd, 11, axis=-1)
        step = maxd / 10
        mine = np.concatenate([np.arange(10)[None, :] * step[:, None], maxd[:, None]], axis=1)
        assert np.array_equal(ref, mine)
    for k in (1, 2, 1040 ** 2, kmax):
        assert np.array_equal(np.linspace(0, np.sqrt(k), 11), hd.ring_bounds(np.sqrt(k), 10))


def get_targets_literal(mask_thresh, mask_contour, nb_layers, centroid_y, centroid_x):
    """quantify_pipline.py:61-91 as written, with skimage's label(connectivity=1) + regionprops centroid spelled as scipy's
    label (cross-shaped structure) + center_of_mass per label (no area filter)."""
    lbl, n = ndimage.label(mask_thresh)
    cen = np.array(ndimage.center_of_mass(np.ones_like(lbl), lbl, np.arange(1, n + 1))).reshape(n, 2)
    cy_all, cx_all = cen[:, 0], cen[:, 1]
    coords = np.where(mask_contour)
    if len(coords[0]) == 0 or len(cx_all) == 0:
        return np.zeros_like(mask_thresh, dtype=np.float32)
    distances = np.sqrt((coords[1] - centroid_x) ** 2 + (coords[0] - centroid_y) ** 2)
    max_distance = np.max(distances)
    ring_bounds = np.linspace(0, max_distance, nb_layers + 1)
    dists_centroids = np.sqrt((np.array(cx_all) - centroid_x) ** 2 + (np.array(cy_all) - centroid_y) ** 2)
    image_ring = np.zeros_like(mask_thresh, dtype=np.float32)
    for i in range(nb_layers):
        in_ring = (ring_bounds[i] < dists_centroids) & (dists_centroids <= ring_bounds[i + 1])
        ring_mask = (ring_bounds[i] < distances) & (distances <= ring_bounds[i + 1])
        if np.any(ring_mask):
            image_ring[coords[0][ring_mask], coords[1][ring_mask]] = np.sum(in_ring)
    return image_ring


def _radial_cases():
    rgb, mask = cell_image(80, 110, 1)
    _, _, roi = hd.roi_mask(rgb)
    cx, cy, _ = hd.roi_centroid(roi)
    yield "cell", mask, roi, cy, cx
    yield "empty_roi", mask, np.zeros_like(roi), 40, 55
    yield "no_droplets", np.zeros_like(mask), roi, cy, cx
    one = np.zeros_like(roi)
    one[30, 40] = 1
    yield "one_pixel_roi", mask, one, 30, 40
    far = np.zeros_like(mask)
    far[0, 0] = far[79, 109] = 1
    small = np.zeros_like(roi)
    small[35:45, 50:60] = 1
    yield "droplets_outside_rings", far, small, 40, 55
    # a droplet centroid at distance exactly 2 = bound 1 of a ROI with maxd 10 (L = 5): it belongs to ring 0, not 1
    m = np.zeros((30, 30), np.uint8)
    m[10, 12] = 1
    m[10, 20] = 1
    r = np.zeros((30, 30), np.uint8)
    r[10, 10:21] = 1
    yield "centroid_on_bound", m, r, 10, 10


@pytest.mark.parametrize("case", list(_radial_cases()), ids=lambda c: c[0])
def test_radial_equals_literal_get_targets(case):
    _, mask, roi, cy, cx = case
    for L in (1, 5, 10):
        img, ring, counts, maxd = hd.radial_map(mask, roi, L, cy, cx)
        ref = get_targets_literal(mask, roi, L, cy, cx)
        assert img.dtype == np.float32 and np.array_equal(img, ref)
        assert ((ring > 0) <= (roi > 0)).all()
    if case[0] == "centroid_on_bound":
        assert hd.radial_map(mask, roi, 5, cy, cx)[2].tolist() == [1, 0, 0, 0, 1]


def test_rings_count_every_component_whatever_min_area():
    """The maps use every 4-connected component (no min_area filter), also where the droplet table drops small ones."""
    import quantify_droplets_batch as q
    rgb, mask = cell_image(60, 90, 2)
    mask[5, 5] = 1                     # an isolated one-pixel droplet
    mask[4:7, 4] = mask[4:7, 6] = mask[4, 5] = mask[6, 5] = 0
    _, _, roi = hd.roi_mask(rgb)
    cx, cy, _ = hd.roi_centroid(roi)
    n_all = ndimage.label(mask)[1]
    assert len(q.quantify(mask, 3, None)) < n_all
    _, _, counts, _ = hd.radial_map(mask, roi, 255, cy, cx)
    ref = get_targets_literal(mask, roi, 255, cy, cx)
    assert np.array_equal(hd.radial_map(mask, roi, 255, cy, cx)[0], ref)
    assert hd.droplet_centroids(mask)[0].shape == (n_all,)


def gaussian_fp64(a, sigma):
    """The HIP kernels' order: axis 0 then 1, centre tap then (a[-j] + a[+j]) w_j from the outermost pair inwards in fp64,
    scipy's "reflect" border at any distance, float32 after each axis."""
    w = hd.gaussian_taps(sigma)
    R = len(w) - 1

    def refl(i, n):
        i = i % (2 * n)
        return np.where(i >= n, 2 * n - 1 - i, i)

    out = a.astype(np.float32)
    for axis in (0, 1):
        v = np.moveaxis(out.astype(np.float64), axis, 0)
        n = v.shape[0]
        acc = np.empty_like(v)
        for y in range(n):
            s = v[y] * w[0]
            for j in range(R, 0, -1):
                s = s + (v[refl(y - j, n)] + v[refl(y + j, n)]) * w[j]
            acc[y] = s
        out = np.moveaxis(acc.astype(np.float32), 0, axis)
    return out


@pytest.mark.parametrize("shape,kernel", [((96, 130), 21), ((5, 300), 21), ((3, 4), 21), ((40, 17), 55)])
def test_spatial_order_equals_scipy_bit_for_bit(shape, kernel):
    rgb, mask = cell_image(*shape, 5) if min(shape) > 10 else (None, (np.random.default_rng(1).random(shape) < .3).astype(np.uint8))
    roi = hd.roi_mask(rgb)[2] if rgb is not None else (np.random.default_rng(2).random(shape) < .6).astype(np.uint8)
    s = kernel / 6
    for plane in (mask, roi):
        assert np.array_equal(gaussian_fp64(plane, s), ndimage.gaussian_filter(plane.astype(np.float32), s))
    ref = hd.spatial_map(mask, roi, kernel)
    mine = gaussian_fp64(mask, s) / (gaussian_fp64(roi, s) + np.float32(1e-5)) * np.float32(100)
    assert ref.dtype == np.float32 and np.array_equal(ref, mine)


@pytest.mark.parametrize("kind", ["ramp", "zero", "constant", "spatial"])
def test_colormap_index_equals_imsave_pixels(kind, tmp_path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    rng = np.random.default_rng(6)
    m = {"ramp": np.linspace(0, 3, 40 * 50, dtype=np.float32).reshape(40, 50) ** 3,
         "zero": np.zeros((20, 30), np.float32),
         "constant": np.full((20, 30), 7.5, np.float32),
         "spatial": hd.spatial_map((rng.random((60, 80)) < .2).astype(np.uint8), (rng.random((60, 80)) < .7).astype(np.uint8))}[kind]
    norm = m                                     # the reference's normalize()
    if m.max() > m.min():
        norm = (m - m.min()) / (m.max() - m.min())
    plt.imsave(tmp_path / "a.png", norm, cmap="hot")
    ref = np.array(Image.open(tmp_path / "a.png"))
    assert np.array_equal(hd.colormap_lut("hot")[hd.colormap_index(m)], ref)
    hd.write_pngs(hd.colormap_index(m), hd.colormap_index(m), tmp_path, "b")
    assert np.array_equal(np.array(Image.open(tmp_path / "b_radial_density.png")), ref)


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_density_abi_rejects_bad_arguments(lib):
    import ctypes
    assert lib.unetdc_version() == 2
    assert lib.unetdc_density_workspace(1040, 1388) > 1040 * 1388 * 20
    assert lib.unetdc_density_workspace(1, 1388) == 0
    taps = hd.gaussian_taps(3.5)
    tp = taps.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every check below fails before any HIP call

    def call(h=64, w=64, layers=10, sigma=3.5, ptr=fake, taps_=tp):
        return lib.unetdc_density_maps(ptr, fake, h, w, fake, fake, fake, fake, 100, layers, sigma, taps_, fake, 1 << 30,
                                       fake, fake, fake, None, None, None, None, None, None)
    cases = [(dict(ptr=None), b"null"), (dict(taps_=None), b"null"), (dict(h=1), b"geometry"), (dict(w=0), b"geometry"),
             (dict(layers=0), b"nb_layers"), (dict(layers=256), b"nb_layers"), (dict(sigma=0.0), b"sigma"),
             (dict(sigma=float("nan")), b"sigma"), (dict(sigma=40.0), b"sigma")]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    rc = lib.unetdc_density_maps(fake, fake, 64, 64, fake, fake, fake, fake, 100, 10, 3.5, tp, fake, 16, fake, fake, fake,
                                 None, None, None, None, None, None)
    assert rc == -3 and b"workspace" in lib.unetdc_last_error()
    assert lib.unetdc_density_sqrt(None, None, 5, None) == -1 and b"density_sqrt" in lib.unetdc_last_error()


def _run_cli(tmp_path, monkeypatch, tag, extra):
    import quantify_droplets_batch as q
    from models.model_2 import UNetDC
    monkeypatch.setattr(q, "DEVICE", "cpu")
    monkeypatch.setattr(q, "IMG_SIZE", 64)
    img_dir = tmp_path / "imgs"
    if not img_dir.exists():
        img_dir.mkdir()
        for i, (h, w) in enumerate([(96, 120), (70, 90), (64, 64)]):
            Image.fromarray(cell_image(h, w, 10 + i)[0]).save(img_dir / f"im{i}.png")
        torch.manual_seed(0)
        torch.save(UNetDC(3, 1).state_dict(), tmp_path / "ck.pth")
    return q.main(["--img_dir", str(img_dir), "--ckpt_path", str(tmp_path / "ck.pth"), "--out_dir", str(tmp_path / tag),
                   "--batch", "2", "--skip_excel", "--skip_histogram", "--background_radius", "15", *extra])


def test_cli_density_maps_cpu(tmp_path, monkeypatch):
    plain = _run_cli(tmp_path, monkeypatch, "plain", [])
    dens = _run_cli(tmp_path, monkeypatch, "dens", ["--density_maps", "--nb_layers", "6"])
    files = lambda d: sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file())
    fp, fd = files(plain), files(dens)
    assert not any("density" in f for f in fp)
    new = sorted(set(fd) - set(fp))
    assert new == sorted(["density_per_image.csv"] + [f"im{i}_{k}_density.png" for i in range(3) for k in ("radial", "spatial")])
    for f in fp:                                     # the files of a run without the flag, unchanged
        assert (plain / f).read_bytes() == (dens / f).read_bytes(), f
    csv = pd.read_csv(dens / "density_per_image.csv", float_precision="round_trip")
    assert list(csv.columns) == ["filename", "roi_area_px", "roi_centroid_x", "roi_centroid_y", "otsu_threshold",
                                 "max_ring_distance_px"] + [f"ring_{i}" for i in range(1, 7)]
    for i in range(3):
        rgb = np.array(Image.open(tmp_path / "imgs" / f"im{i}.png").convert("RGB"))
        mask = (np.array(Image.open(dens / "predicted_masks" / f"im{i}_pred.png")) > 0).astype(np.uint8)
        r = hd.density_maps(rgb, mask, 6, 21)
        row = csv.iloc[i]
        assert row["filename"] == f"im{i}.png" and row["roi_area_px"] == r["roi_area"] and row["otsu_threshold"] == r["threshold"]
        assert row["max_ring_distance_px"] == r["max_ring_distance"]
        lut = hd.colormap_lut("hot")
        for k in ("radial", "spatial"):
            assert np.array_equal(np.array(Image.open(dens / f"im{i}_{k}_density.png")), lut[r[f"{k}_index"]])


def test_cli_rejects_density_settings_the_kernels_cannot_run(tmp_path, monkeypatch):
    """--density_kernel 193 means a Gaussian radius of 129 > 128: refused before any image, on the CPU path as on the device."""
    assert int(4 * 192 / 6 + 0.5) == 128 and int(4 * 193 / 6 + 0.5) == 129
    for bad in (["--density_kernel", "193"], ["--density_kernel", "0"], ["--nb_layers", "0"], ["--nb_layers", "256"]):
        with pytest.raises(SystemExit):
            _run_cli(tmp_path, monkeypatch, "bad", ["--density_maps", *bad])
        assert not list((tmp_path / "bad").glob("*.csv"))
