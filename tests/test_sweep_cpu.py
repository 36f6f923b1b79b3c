"""CPU: the host path of the threshold sweep (utils/threshold_sweep.py) against the slow restatement
of the same definition (tests/sweep_ref.py), the monotonicity the histogram form rests on, the derived numbers of
sweep_table on hand-computed tables, the argument checks of the script, and --calibrate_thresh on the CPU path."""
import functools

import numpy as np
import pytest

from tests.sweep_ref import sweep_ref
from utils import threshold_sweep as ts

# (name, (ph, pw), (oh, ow), linear): nearest identity, nearest downscale, linear upscale with edge taps on every side, and
# the anisotropy of 512^2 -> 1040 x 1388
GEOMETRIES = (("nearest_identity", (33, 65), (33, 65), False), ("nearest_down", (40, 40), (17, 23), False),
              ("linear_up_edges", (7, 5), (13, 9), True), ("linear_aniso", (64, 64), (130, 173), True))
KS = (1, 2, 10, 100, 1024)


def edge_probs(ph, pw, K, seed, n=1):
    """fp32 [n][ph][pw]: uniform noise with a third of the pixels replaced by the values that decide a comparison: exact grid
    values (a pixel equal to t_k is not set at k), their fp32 neighbours on both sides, 0, -0, 1, values above 1, a denormal,
    infinities, a negative value and NaN."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, ph, pw), dtype=np.float32)
    g = ts.grid(K)
    special = np.concatenate([g, np.nextafter(g, np.float32(2)), np.nextafter(g, np.float32(-1)),
                              np.array([0.0, -0.0, 1.0, 1.5, 3e38, 1e-45, 1e-39, np.inf, -np.inf, -0.25, np.nan], np.float32)])
    pick = rng.random(p.shape) < 1 / 3
    p[pick] = rng.choice(special, int(pick.sum()))
    for img in p.reshape(n, -1):                      # every value of the fixed list at least once per image, where it fits
        k = min(len(img), 11)
        img[rng.choice(len(img), k, replace=False)] = special[-11:][:k]
    return p


def gt_of(oh, ow, seed, n=1):
    """uint8 [n][oh][ow]: blocks of annotation; nonzero values other than 255 count as annotated too."""
    rng = np.random.default_rng(1000 + seed)
    g = (rng.random((n, (oh + 3) // 4, (ow + 3) // 4)) < 0.4).repeat(4, axis=1).repeat(4, axis=2)[:, :oh, :ow]
    return (g * rng.choice(np.array([255, 1, 7], np.uint8), g.shape)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference_hist(name, K, image=0):
    """sweep_ref on image `image` of a geometry's fixture (computed once per session; tests must not change it)."""
    _, (ph, pw), (oh, ow), linear = next(geo for geo in GEOMETRIES if geo[0] == name)
    h = sweep_ref(edge_probs(ph, pw, K, seed=K, n=3)[image], gt_of(oh, ow, seed=K, n=3)[image], (oh, ow), K, linear)
    h.setflags(write=False)
    return h


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_host_path_equals_restatement(geo, K):
    name, (ph, pw), (oh, ow), linear = geo
    p, g = edge_probs(ph, pw, K, seed=K, n=3)[0], gt_of(oh, ow, seed=K, n=3)[0]
    assert np.isnan(p).any() and (p == 0).any() and (p > 1).any()
    h = ts.sweep_hist_numpy(p, g, (oh, ow), K, linear=linear)
    assert h.dtype == np.int64 and h.shape == (2, K + 1) and h.sum() == oh * ow
    assert np.array_equal(h, reference_hist(name, K))
    assert h[0].sum() == int((g == 0).sum()) and h[:, 1:].sum() > 0 and h[:, 0].sum() > 0


@pytest.mark.parametrize("K", (1, 10, 100))
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_histogram_tail_sums_are_the_counts_of_each_mask(geo, K):
    """Monotonicity, directly: for every k the pixels of level > k are exactly the pixels of mask_k, per annotation class."""
    from unet_dc_segmentation_amd.droplets import resize_mask_like_reference, resize_nearest_cv2
    name, (ph, pw), (oh, ow), linear = geo
    p, g = edge_probs(ph, pw, K, seed=K, n=3)[0], gt_of(oh, ow, seed=K, n=3)[0] != 0
    h = ts.sweep_hist_numpy(p, g, (oh, ow), K, linear=linear)
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(ts.grid(K)):
            m512 = (p > t).astype(np.uint8)
            m = (resize_mask_like_reference(m512, ow, oh) if linear else resize_nearest_cv2(m512, ow, oh)) != 0
            assert h[1, k + 1:].sum() == int((m & g).sum()) and h[0, k + 1:].sum() == int((m & ~g).sum()), k


def test_special_values_land_where_the_definition_puts_them():
    K = 10
    g = ts.grid(K)
    vals = np.array([[0.0, -0.0, np.nan, -1.0, 1e-45, g[3], np.nextafter(g[3], np.float32(1)), 1.0, 1.5, np.inf]], np.float32)
    want = [0, 0, 0, 0, 1, 3, 4, K, K, K]                      # a pixel equal to t_3 is set at k = 0, 1, 2 only
    for j, lev in enumerate(want):
        h = ts.sweep_hist_numpy(vals[:, j:j + 1], np.ones((1, 1), np.uint8), (1, 1), K, linear=False)
        assert h[1, lev] == 1 and h.sum() == 1, (j, lev)
        assert np.array_equal(h, sweep_ref(vals[:, j:j + 1], np.ones((1, 1), np.uint8), (1, 1), K, False))


def test_grid_is_the_fp32_division():
    bits = lambda v: np.asarray(v, np.float32).view(np.uint32)      # noqa: E731
    assert bits(ts.grid(10)[3]) == bits(np.float32(0.3)) and bits(ts.grid(100)[30]) == bits(np.float32(0.3))
    for K in KS:
        g = ts.grid(K)
        assert g.dtype == np.float32 and len(g) == K and g[0] == 0 and np.all(np.diff(g) > 0) and g[-1] < 1
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError):
            ts.grid(bad)


def test_sweep_table_hand_computed():
    t = ts.sweep_table([[5, 3, 2], [1, 2, 4]])
    assert t["K"] == 2 and t["threshold"].tolist() == [0.0, 0.5]
    assert t["tp"].tolist() == [6, 4] and t["fp"].tolist() == [5, 2] and t["fn"].tolist() == [1, 3] and t["tn"].tolist() == [5, 8]
    assert t["precision"].tolist() == [6 / 11, 4 / 6] and t["recall"].tolist() == [6 / 7, 4 / 7]
    assert t["dice"].tolist() == [12 / 18, 8 / 13] and t["iou"].tolist() == [6 / 12, 4 / 9]
    assert t["average_precision"] == (6 / 7 - 4 / 7) * (6 / 11) + (4 / 7 - 0.0) * (4 / 6)
    assert t["best_dice_k"] == 0 and t["best_iou_k"] == 0
    rows = ts.table_rows([[5, 3, 2], [1, 2, 4]])
    assert [list(r) for r in rows] == [list(ts.COLUMNS)] * 2
    assert rows[1] == {"k": 1, "threshold": 0.5, "tp": 4, "fp": 2, "fn": 3, "tn": 8, "precision": 4 / 6, "recall": 4 / 7,
                       "dice": 8 / 13, "iou": 4 / 9}
    assert all(type(rows[0][c]) is int for c in ("k", "tp", "fp", "fn", "tn"))


def test_sweep_table_zero_denominators_and_ties():
    ratios = ("precision", "recall", "dice", "iou")
    t = ts.sweep_table([[10, 0, 0], [0, 0, 0]])                  # nothing annotated, nothing predicted: every ratio 1.0
    assert all(t[q].tolist() == [1.0, 1.0] for q in ratios) and t["average_precision"] == 1.0 and t["best_dice_k"] == 0
    t = ts.sweep_table([[10, 0, 0], [4, 0, 0]])                  # annotated, never predicted: every denominator-free ratio 0.0
    assert all(t[q].tolist() == [0.0, 0.0] for q in ratios) and t["average_precision"] == 0.0
    t = ts.sweep_table([[3, 0, 7], [0, 0, 0]])                   # predicted, nothing annotated: recall has no denominator
    assert all(t[q].tolist() == [0.0, 0.0] for q in ratios) and t["fp"].tolist() == [7, 7]
    t = ts.sweep_table([[3, 7, 0], [0, 0, 0]])                   # the all-empty rule holds per k: predicted at k = 0 only
    assert t["precision"].tolist() == [0.0, 1.0] and t["dice"].tolist() == [0.0, 1.0] and t["best_dice_k"] == 1
    t = ts.sweep_table([[0, 5, 0, 0], [0, 0, 0, 5]])             # dice 2/3, 1, 1: the smallest k of the maximum
    assert t["dice"].tolist() == [10 / 15, 1.0, 1.0] and t["best_dice_k"] == 1 and t["best_iou_k"] == 1
    with pytest.raises(ValueError):
        ts.sweep_table([1, 2, 3])


def test_script_refuses_bad_sweep_arguments(tmp_path):
    import quantify_droplets_batch as q
    base = ["--img_dir", str(tmp_path / "none"), "--out_dir", str(tmp_path / "out")]
    for extra, word in ((["--thresh_sweep"], "--gt_dir"), (["--thresh_sweep", "10", "--sweep_objects", "0.4"], "--gt_dir"),
                        (["--gt_dir", "g", "--sweep_objects", "0.4"], "--thresh_sweep"),
                        (["--gt_dir", "g", "--thresh_sweep", "0"], "1..1024"),
                        (["--gt_dir", "g", "--thresh_sweep", "1025"], "1..1024"),
                        (["--gt_dir", "g", "--thresh_sweep", "--sweep_objects", "0.4,x"], "commas"),
                        (["--gt_dir", "g", "--thresh_sweep", "--prob_thresh_low", "0.2", "--sweep_objects", "0.3,0.1"],
                         "--prob_thresh_low")):
        with pytest.raises(SystemExit) as e:
            q.main(base + extra)
        assert word in str(e.value), (extra, e.value)
        assert not (tmp_path / "out").exists()
    a = q.build_parser().parse_args(base + ["--gt_dir", "g", "--thresh_sweep"])
    assert a.thresh_sweep == 100 and q.sweep_options(a)["objects"] == []
    a = q.build_parser().parse_args(base + ["--gt_dir", "g", "--thresh_sweep", "7", "--prob_thresh_low", "0.2", "--sweep_objects", "0.2,0.5"])
    assert a.thresh_sweep == 7 and q.sweep_options(a)["objects"] == [0.2, 0.5]
    assert q.sweep_options(q.build_parser().parse_args(base)) is None


def test_cli_sweep_on_the_cpu_path(tmp_path, monkeypatch, capsys):
    """--thresh_sweep / --sweep_objects on the CPU path: the pooled table is sweep_table of the summed per-image histograms,
    the object row at --prob_thresh is the ALL row of match_per_image.csv, and no other output changes."""
    import pandas as pd
    from PIL import Image
    from tests.test_split_cpu import SIZE, cli_probs, files, noise_mask, run_cli
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    gts = [noise_mask(SIZE, SIZE, seed=90 + i, sigma=3.0, frac=0.3) for i in range(3)]
    for i, g in enumerate(gts):
        Image.fromarray(g * 255).save(gt_dir / f"im{i}.png")
    args = ["--min_area", "2", "--gt_dir", str(gt_dir), "--prob_thresh_low", "0.15", "--fill_holes"]
    plain = run_cli(tmp_path, monkeypatch, "plain", args)
    out = run_cli(tmp_path, monkeypatch, "sweep", args + ["--thresh_sweep", "10", "--sweep_objects", "0.5,0.85"])
    assert sorted(set(files(out)) - set(files(plain))) == ["threshold_sweep.csv", "threshold_sweep_objects.csv"]
    for f in files(plain):
        assert (plain / f).read_bytes() == (out / f).read_bytes(), f
    hist = sum(ts.sweep_hist_numpy(cli_probs()[i, 0].numpy(), gts[i], (SIZE, SIZE), 10) for i in range(3))
    t = pd.read_csv(out / "threshold_sweep.csv", float_precision="round_trip")
    assert list(t.columns) == list(ts.COLUMNS) and t.to_dict("records") == ts.table_rows(hist)
    assert t["tp"][0] + t["fn"][0] == sum(int(g.sum()) for g in gts) and (t["tp"] + t["fp"] + t["fn"] + t["tn"] == 3 * SIZE * SIZE).all()
    o = pd.read_csv(out / "threshold_sweep_objects.csv", float_precision="round_trip")
    m = pd.read_csv(out / "match_per_image.csv", float_precision="round_trip")
    assert o["threshold"].tolist() == [0.5, 0.85] and list(o.columns)[1:] == list(m.columns)[1:]
    assert o.iloc[0, 1:].tolist() == m[m["filename"] == "ALL"].iloc[0, 1:].tolist()
    assert o["n_pred"][1] < o["n_pred"][0]                     # 0.85 keeps the discs of image 0 (0.9) and drops the noise (0.8)
    assert "best pooled Dice" in capsys.readouterr().out


TRAIN_ARGS = ["--synthetic", "--synthetic_len", "10", "--img_size", "32", "--batch", "2", "--epochs", "1", "--steps", "1",
              "--workers", "0", "--in_channels", "1", "--device", "cpu"]


def test_calibrate_thresh_on_the_cpu_path(tmp_path, capsys):
    import train_DC_focal as t
    ck = str(tmp_path / "ck.pth")
    hist = t.main(TRAIN_ARGS + ["--ckpt_path", ck, "--calibrate_thresh", "10"])
    c = hist.calibration
    assert set(c) == {"K", "best_dice_threshold", "best_dice", "average_precision", "hist"} and c["K"] == 10
    assert c["hist"].shape == (2, 11) and c["hist"].dtype == np.int64
    assert c["hist"].sum() == 2 * 32 * 32                      # the validation split: 10 // 5 images
    table = ts.sweep_table(c["hist"])
    assert c["best_dice"] == table["dice"].max() and c["best_dice_threshold"] == table["threshold"][table["best_dice_k"]]
    assert "Threshold calibration" in capsys.readouterr().out
    plain = t.main(TRAIN_ARGS + ["--ckpt_path", ck])
    assert getattr(plain, "calibration", None) is None
    assert t.build_parser().parse_args(["--calibrate_thresh"]).calibrate_thresh == 100
    with pytest.raises(SystemExit):
        t.main(TRAIN_ARGS + ["--ckpt_path", ck, "--calibrate_thresh", "2000"])
