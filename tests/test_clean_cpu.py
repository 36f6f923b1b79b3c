"""CPU: the host path of the mask-cleaning stage (utils/droplet_clean.py) against the plain-loop restatement of DESIGN.md
section 13 (tests/clean_ref.py) and scipy's binary_fill_holes, the properties the definition promises, the argument checks of
unetdc_mask_clean, and quantify_droplets_batch.py --prob_thresh_low / --fill_holes on its CPU path.  Exact equality only."""
import numpy as np
import pandas as pd
import pytest
from PIL import Image
from scipy import ndimage

from tests.clean_ref import clean_ref, components, named_cases, noise, spiral, weak_for
from tests.test_split_cpu import SIZE, FixedProbs, cli_probs, files, noise_mask, run_cli  # noqa: F401
from utils.droplet_clean import COUNT_NAMES, clean_mask

CASES = named_cases()


def assert_equals_restatement(strong, weak, limit):
    m, c = clean_mask(strong, weak, limit)
    rm, rc = clean_ref(strong, weak, limit)
    assert m.dtype == np.uint8 and np.array_equal(m, rm)
    assert c.dtype == np.int64 and c.tolist() == rc
    return m, rc


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_path_equals_restatement_on_named_cases(name):
    strong, weak, limit = CASES[name]
    assert_equals_restatement(strong, weak, limit)
    w2 = weak if weak is not None else weak_for(strong)
    for lim in (0, 1, 5, -1):
        assert_equals_restatement(strong, None, lim)
        assert_equals_restatement(strong, w2, lim)


def test_named_cases_say_what_their_names_say():
    r = {k: clean_ref(*v) for k, v in CASES.items()}
    assert r["1x1_bg"][0].tolist() == [[0]] and r["1x1_fg"][0].tolist() == [[1]]
    assert r["1x7"][0].tolist() == [[1, 1, 1, 0, 1, 1, 0]] and r["1x7"][1] == [2, 0, 0, 0]
    assert np.array_equal(r["7x1"][0], r["1x7"][0].T)
    assert not r["all_zero"][0].any() and r["all_one"][0].all()
    assert r["hole_3x3"][0].all() and r["hole_3x3"][1] == [0, 1, 1, 0]
    m = r["hole_open_to_border"][0]
    assert m[1, 1] == 0 and m[4, 1] == 0 and m[3, 3] == 1 and r["hole_open_to_border"][1] == [0, 1, 1, 0]
    assert r["diamond_ring"][0][1:3, 1:3].all() and r["diamond_ring"][1] == [0, 1, 4, 0]        # the diagonal leak is a hole
    assert r["diamond_ring"][0][0, 0] == 0
    ring = r["droplet_in_hole_in_ring"]
    assert ring[0][1:10, 1:11].all() and ring[1][1] == 2                                        # the moat and the inner hole
    assert ndimage.label(ring[0])[1] == 1 and ndimage.label(CASES["droplet_in_hole_in_ring"][0])[1] == 2
    two = r["holes_N_and_N_plus_1"]
    assert two[1] == [0, 1, 4, 1] and two[0][2, 2] == 1 and two[0][2, 6] == 0
    assert np.array_equal(r["seed_is_last_pixel"][0], CASES["seed_is_last_pixel"][1]) and r["seed_is_last_pixel"][1][0] == 5
    assert not r["weak_without_strong"][0].any()
    d = r["diagonal_weak_components"][0]
    assert d[:2, :2].all() and d.sum() == 4
    o = r["strong_outside_weak"]
    assert o[0][3, 4] == 0 and o[0].sum() == 3 and o[1][0] == 2
    assert np.array_equal(r["weak_equals_strong"][0], CASES["weak_equals_strong"][0]) and r["weak_equals_strong"][1][0] == 0
    sp = spiral(64)
    assert len(components(sp.astype(bool).tolist())) == 1 and len(components((sp == 0).tolist())) == 1 and sp.sum() > 1500
    assert np.array_equal(r["spiral_foreground"][0], sp) and r["spiral_foreground"][1] == [int(sp.sum()) - 1, 0, 0, 0]
    assert np.array_equal(r["spiral_background"][0], 1 - sp)
    assert CASES["noise_37x83"][0].shape == (37, 83) and r["noise_37x83"][1][3] > 0 and r["noise_37x83"][1][1] > 0


def test_host_path_equals_restatement_on_random_small_masks():
    rng = np.random.default_rng(3)
    for k in range(300):
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        weak = (rng.random((h, w)) < rng.uniform(0.2, 0.9)).astype(np.uint8)
        strong = (rng.random((h, w)) < 0.25).astype(np.uint8)
        if k % 3:
            strong &= weak                                # two in three nested, as the script makes them
        assert_equals_restatement(strong, weak if k % 5 else None, (0, -1, 1, 2, 3, 7)[k % 6])


def test_unlimited_filling_is_scipy_binary_fill_holes():
    rng = np.random.default_rng(4)
    for k in range(300):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        m = (rng.random((h, w)) < rng.uniform(0.3, 0.8)).astype(np.uint8)
        got, c = clean_mask(m, None, -1)
        assert np.array_equal(got, ndimage.binary_fill_holes(m).astype(np.uint8))
        assert c[0] == 0 and c[3] == 0 and c[2] == got.sum() - m.sum()
    for name, (strong, _, _) in CASES.items():
        assert np.array_equal(clean_mask(strong, None, -1)[0], ndimage.binary_fill_holes(strong).astype(np.uint8)), name
    big = noise_mask(276, 408, seed=1)
    assert np.array_equal(clean_mask(big, None, -1)[0], ndimage.binary_fill_holes(big).astype(np.uint8))


def test_hysteresis_is_idempotent_and_the_identity_for_equal_masks():
    for seed in range(20):
        weak = noise_mask(40, 57, seed=seed, sigma=1.5, frac=0.5)
        strong = weak & noise(40, 57, 100 + seed, 0.05)
        m, c = clean_mask(strong, weak, 0)
        assert np.all(m >= strong) and np.all(m <= weak) and 0 < m.sum() < weak.sum()
        again, c2 = clean_mask(m, weak, 0)
        assert np.array_equal(again, m) and c2.tolist() == [0, 0, 0, 0]
        same, c3 = clean_mask(weak, weak, 0)
        assert np.array_equal(same, weak) and c3.tolist() == [0, 0, 0, 0]


def test_counts_add_up():
    """With strong inside weak (the script's case): pixels of the result = pixels of strong + added + filled."""
    for seed in range(20):
        weak = noise_mask(40, 57, seed=seed, sigma=1.5, frac=0.5)
        strong = weak & noise(40, 57, 100 + seed, 0.1)
        for lim in (0, 2, 9, -1):
            for wk in (weak, None):
                m, c = clean_mask(strong, wk, lim)
                assert int(m.sum()) == int(strong.sum()) + c[0] + c[2]
                assert (c[1] == 0) == (c[2] == 0) and c[2] >= c[1] and (lim > 0 or c[3] == 0)
                if lim > 0:
                    assert c[2] <= lim * c[1]


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_mask_clean_abi_rejects_bad_arguments_before_any_launch(lib):
    import ctypes
    assert lib.unetdc_mask_clean_workspace(1040, 1388) == 8 * 1040 * 1388 + 64
    assert lib.unetdc_mask_clean_workspace(0, 5) == 0 and lib.unetdc_mask_clean_workspace(5, 16385) == 0
    n = 64 * 64
    a, b, o, ws, cnt = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20))   # never dereferenced

    def clean(strong=a, weak=b, h=64, w=64, limit=-1, ws_=ws, bytes_=1 << 19, out=o, counts=cnt):
        return lib.unetdc_mask_clean(strong, weak, h, w, limit, ws_, bytes_, out, counts, None)
    for kw, msg in [(dict(strong=None), b"null"), (dict(out=None), b"null"), (dict(ws_=None), b"null"), (dict(h=0), b"geometry"),
                    (dict(w=16385), b"geometry"), (dict(h=-3), b"geometry"),
                    (dict(bytes_=lib.unetdc_mask_clean_workspace(64, 64) - 1), b"workspace too small"),
                    (dict(out=ctypes.c_void_p((1 << 20) + 5)), b"overlap"), (dict(out=ctypes.c_void_p((2 << 20) - 1)), b"overlap"),
                    (dict(out=ctypes.c_void_p((2 << 20) + n - 1)), b"overlap"), (dict(out=ctypes.c_void_p((4 << 20) + 8 * n)), b"overlap"),
                    (dict(counts=ctypes.c_void_p((3 << 20) + 8)), b"overlap"), (dict(ws_=ctypes.c_void_p((4 << 20) + 2)), b"aligned")]:
        assert clean(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())


# ---- quantify_droplets_batch.py on the CPU path --------------------------------------------------------------------------
def ring_probs():
    """Three 64 x 64 maps: a ring (rim 0.9, core 0.1) beside a faint disc (core 0.9, skirt 0.4); noise at two levels; nothing."""
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    r1 = (yy - 22) ** 2 + (xx - 20) ** 2
    r2 = (yy - 44) ** 2 + (xx - 45) ** 2
    p0 = np.full((SIZE, SIZE), 0.1)
    p0[(r1 <= 100) & (r1 > 25)] = 0.9
    p0[r2 <= 100] = 0.4
    p0[r2 <= 9] = 0.9
    nz = noise_mask(SIZE, SIZE, 2)
    p1 = np.where(nz > 0, 0.4, 0.1)
    p1[(nz > 0) & (noise(SIZE, SIZE, 3, 0.2) > 0)] = 0.8
    return np.stack([p0, p1, np.full((SIZE, SIZE), 0.1)]).astype(np.float32)


def test_cli_flags_parse_and_a_bad_low_threshold_is_refused(tmp_path, monkeypatch):
    import quantify_droplets_batch as q
    p = q.build_parser()
    a = p.parse_args(["--img_dir", "x"])
    assert a.prob_thresh_low is None and a.fill_holes == 0 and q.clean_options(a) is None
    a = p.parse_args(["--img_dir", "x", "--fill_holes"])
    assert a.fill_holes == -1 and q.clean_options(a) == {"low": None, "holes": -1, "rows": []}
    a = p.parse_args(["--img_dir", "x", "--fill_holes", "12", "--prob_thresh_low", "0.1"])
    assert a.fill_holes == 12 and q.clean_options(a) == {"low": 0.1, "holes": 12, "rows": []}
    a = p.parse_args(["--img_dir", "x", "--prob_thresh", "0.4", "--prob_thresh_low", "0.4"])
    assert q.clean_options(a) is None                        # equal: the option is a no-op
    for bad in (["--prob_thresh_low", "0.6"], ["--prob_thresh_low", "nan"], ["--fill_holes", "-7"]):
        with pytest.raises(SystemExit):
            run_cli(tmp_path, monkeypatch, "bad", bad)       # --prob_thresh is 0.5 there
        assert not (tmp_path / "bad").exists()


def test_cli_cleaning_on_the_cpu_path(tmp_path, monkeypatch):
    import torch
    import quantify_droplets_batch as q
    probs = ring_probs()
    pt = torch.from_numpy(probs)[:, None]
    plain = run_cli(tmp_path, monkeypatch, "plain", ["--save_overlays"], probs=pt)
    same = run_cli(tmp_path, monkeypatch, "same", ["--save_overlays", "--prob_thresh_low", "0.5"], probs=pt)
    assert files(plain) == files(same) and "mask_clean_per_image.csv" not in files(plain)
    for f in files(plain):
        assert (plain / f).read_bytes() == (same / f).read_bytes(), f
    out = run_cli(tmp_path, monkeypatch, "clean", ["--save_overlays", "--prob_thresh_low", "0.3", "--fill_holes"], probs=pt)
    assert sorted(set(files(out)) - set(files(plain))) == ["mask_clean_per_image.csv"]
    counts = pd.read_csv(out / "mask_clean_per_image.csv")
    assert list(counts.columns) == ["filename", *COUNT_NAMES] and counts["filename"].tolist() == ["im0.png", "im1.png", "im2.png"]
    for i in range(3):
        strong, weak = (probs[i] > 0.5).astype(np.uint8), (probs[i] > 0.3).astype(np.uint8)
        m, c = clean_ref(strong, weak, -1)
        assert np.array_equal(np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")), m * 255)
        assert counts.iloc[i, 1:].tolist() == c
        ref = q.quantify(m, 1, None)                        # the tables are those of quantify on the cleaned mask
        if ref.empty:
            assert not m.any()
            continue
        got = pd.read_csv(out / f"im{i}_droplets.csv", float_precision="round_trip")
        assert list(got.columns) == ["filename"] + list(ref.columns)
        for col in ref.columns:
            assert np.array_equal(got[col].to_numpy(), ref[col].to_numpy()), col
    hole = int(((np.mgrid[0:SIZE, 0:SIZE][0] - 22) ** 2 + (np.mgrid[0:SIZE, 0:SIZE][1] - 20) ** 2 <= 25).sum())
    t0, t1 = pd.read_csv(plain / "im0_droplets.csv"), pd.read_csv(out / "im0_droplets.csv")
    assert len(t0) == len(t1) == 2 and counts[COUNT_NAMES[1]][0] == 1 and counts[COUNT_NAMES[2]][0] == hole
    assert t1["area"][0] == t0["area"][0] + hole                                # the ring became a disc
    assert t1["area"][1] == int((probs[0] > 0.3).sum()) - t0["area"][0] > t0["area"][1]      # the faint disc got its skirt back
    assert list(pd.read_csv(out / "summary_per_image.csv").columns) == list(pd.read_csv(plain / "summary_per_image.csv").columns)
    assert pd.read_csv(out / "summary_per_image.csv")["total_area_px"].tolist() == [int(clean_ref((probs[i] > 0.5), (probs[i] > 0.3), -1)[0].sum()) for i in range(3)]
    # every other consumer sees the cleaned mask too: --split_touching, --droplet_shape and --density_maps on the CPU path
    extra = ["--split_touching", "--droplet_shape", "--density_maps", "--prob_thresh_low", "0.3", "--fill_holes", "40"]
    full = run_cli(tmp_path, monkeypatch, "full", extra, probs=pt)
    from utils.density import rgb_to_gray
    for i in range(2):
        m = clean_ref((probs[i] > 0.5), (probs[i] > 0.3), 40)[0]
        gray = rgb_to_gray(np.array(Image.open(tmp_path / "imgs" / f"im{i}.png").convert("RGB")))
        ref, lab = q.quantify_shape(m, 1, None, 2.0, gray)
        got = pd.read_csv(full / f"im{i}_droplets.csv", float_precision="round_trip")
        assert np.array_equal(got["area"].to_numpy(), ref["area"].to_numpy()) and np.array_equal(got["perimeter"].to_numpy(), ref["perimeter"].to_numpy())
        assert np.array_equal(np.array(Image.open(full / "predicted_masks" / f"im{i}_labels.png")), lab)
        assert np.array_equal(np.array(Image.open(full / "predicted_masks" / f"im{i}_pred.png")), m * 255)
