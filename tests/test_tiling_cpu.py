"""CPU: tiled inference at native resolution -- the tile plan, the reflect-101 fold, the numpy
restatement of the gather and blend kernels (utils/tiling.py), predict_tiled_cpu and the --tile route of
quantify_droplets_batch.py on the CPU path."""
import numpy as np
import pytest
import torch

from utils import tiling as tl


# ---- plan ------------------------------------------------------------------------------------------------------------------
def test_plan_known_answers():
    assert tl.axis_origins(1040, 512, 64) == [0, 264, 528]
    assert tl.axis_origins(1388, 512, 64) == [0, 438, 876]
    yo, xo = tl.tile_plan(1040, 1388, 512, 64)
    assert (yo, xo) == ([0, 264, 528], [0, 438, 876]) and len(yo) * len(xo) == 9


PLAN_SWEEP = [(T, O) for T in (32, 48, 64, 512) for O in sorted({0, 1, 7, 16, T // 2 - 1, T // 2})]


@pytest.mark.parametrize("T,O", PLAN_SWEEP)
def test_plan_properties(T, O):
    dims = sorted({1, 2, T - 1, T, T + 1, T + 2, 2 * T - O - 1, 2 * T - O, 2 * T - O + 1, 2 * T, 3 * T - 2 * O, 3 * T - 2 * O + 1,
                   5 * T + 3, 1040, 1388, 4099})
    for dim in dims:
        o = tl.axis_origins(dim, T, O)
        n = len(o)
        assert o[0] == 0 and o[-1] == max(0, dim - T), (dim, o)
        assert all(b > a for a, b in zip(o, o[1:])), (dim, o)                      # strictly increasing
        assert all(a + T - b >= O for a, b in zip(o, o[1:])), (dim, o)             # every overlap at least O
        if dim <= T:
            assert o == [0]
        else:                                                                      # n is minimal: n - 1 tiles that overlap by
            assert (n - 1) * T - (n - 2) * O < dim <= n * T - (n - 1) * O, (dim, n)   # at least O reach (n-1) T - (n-2) O pixels
        covered = np.zeros(dim, bool)
        for a in o:
            covered[a:a + T] = True
        assert covered.all()


def test_plan_limits():
    for T, O in ((31, 0), (40, 8), (16, 4), (4112, 64), (64, 33), (64, -1)):
        with pytest.raises(ValueError):
            tl.tile_plan(100, 100, T, O)
    with pytest.raises(ValueError):
        tl.axis_origins(0, 64, 16)
    assert tl.tile_plan(100, 96, 64, 32) == ([0, 18, 36], [0, 32])          # T / 2 is allowed


# ---- fold ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (1, 2, 3, 5, 9, 37))
def test_fold_is_numpy_reflect_padding(dim):
    a = np.arange(dim)
    for before, after in ((0, 3), (4, 0), (dim - 1, dim - 1), (3 * dim + 2, 5 * dim + 1), (40, 64)):     # wider than dim - 1 too
        want = np.pad(a, (before, after), mode="reflect")
        got = tl.fold(np.arange(-before, dim + after), dim)
        assert np.array_equal(got, want), (dim, before, after)
    assert tl.fold(7, dim) == tl.fold(np.array([7]), dim)[0] and 0 <= int(tl.fold(-10 ** 6, dim)) < dim


def test_weights():
    assert tl.axis_weights(32, 8).tolist() == [1, 2, 3, 4, 5, 6, 7] + [8] * 18 + [7, 6, 5, 4, 3, 2, 1]
    assert tl.axis_weights(32, 0).tolist() == [1] * 32 and tl.axis_weights(32, 1).tolist() == [1] * 32
    assert tl.axis_weights(32, 16).tolist() == list(range(1, 17)) + list(range(16, 0, -1))


# ---- gather / blend ----------------------------------------------------------------------------------------------------------
GEOMETRIES = [(37, 53, 3, 32, 8), (20, 70, 3, 32, 16), (5, 9, 1, 32, 0), (1, 1, 3, 32, 4), (64, 64, 2, 64, 16), (65, 64, 1, 64, 16),
              (100, 150, 3, 64, 16), (90, 47, 1, 48, 13)]


def image(h, w, c, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c)).astype(np.uint8)


@pytest.mark.parametrize("h,w,c,T,O", GEOMETRIES)
def test_gather_is_the_padded_image_cut_at_the_origins(h, w, c, T, O):
    x = image(h, w, c, seed=h)
    tiles = tl.gather_numpy(x, T, O)
    yo, xo = tl.tile_plan(h, w, T, O)
    assert tiles.shape == (len(yo) * len(xo), c, T, T) and tiles.dtype == np.float32
    if h >= 2 and w >= 2:
        padded = np.pad(x, ((0, max(0, T - h)), (0, max(0, T - w)), (0, 0)), mode="reflect")
    else:
        padded = np.broadcast_to(x[:1, :1], (T, T, c)) if h == 1 and w == 1 else None
    for ty, y0 in enumerate(yo):
        for tx, x0 in enumerate(xo):
            want = padded[y0:y0 + T, x0:x0 + T].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
            assert np.array_equal(tiles[ty * len(xo) + tx].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("h,w,c,T,O", GEOMETRIES)
def test_exact_round_trip(h, w, c, T, O):
    """blend(gather(x)) == x bit for bit.  Values k / 255 are not dyadic, so the tiles are cut from k / 256 instead: with weights
    wy wx <= 16^2 = 2^8 (O <= 16) and at most 16 covering tiles every product k wy wx and every partial sum is an integer below
    2^24 over 2^8, so no fp32 operation rounds, and the division of two such numbers whose quotient k / 256 is representable
    is exact.  Any origin, offset or order error shows."""
    assert O <= 16
    x = image(h, w, c, seed=w)
    yo, xo = tl.tile_plan(h, w, T, O)
    assert all(sum(1 for a in o if a <= i < a + T) <= 4 for o, dim in ((yo, h), (xo, w)) for i in range(dim))     # <= 16 covering tiles
    r = np.arange(T)
    for ch in range(c):
        plane = x[..., ch].astype(np.float32) / np.float32(256)
        tiles = np.stack([plane[tl.fold(y0 + r, h)][:, tl.fold(x0 + r, w)] for y0 in yo for x0 in xo])
        got = tl.blend_numpy(tiles, h, w, T, O)
        assert got.dtype == np.float32 and got.shape == (h, w)
        assert np.array_equal(got.view(np.uint32), plane.view(np.uint32))
        # the gathered k / 255 tiles come back to within the two roundings of one product and one division per covering tile
        back = tl.blend_numpy(tl.gather_numpy(x, T, O)[:, ch], h, w, T, O)
        assert np.abs(back.astype(np.float64) - x[..., ch] / 255.0).max() < 1e-6


@pytest.mark.parametrize("h,w,c,T,O", GEOMETRIES)
def test_blend_accuracy_and_constant(h, w, c, T, O):
    """fp32 against fp64: at most 16 products, 15 adds per sum and one division of values in [0, 1], each within 2^-24 relative:
    far inside 1e-6 absolute."""
    yo, xo = tl.tile_plan(h, w, T, O)
    tiles = np.random.default_rng(T + O).random((len(yo) * len(xo), T, T)).astype(np.float32)
    a, b = tl.blend_numpy(tiles, h, w, T, O), tl.blend_numpy64(tiles, h, w, T, O)
    assert b.dtype == np.float64 and np.abs(a - b).max() < 1e-6
    assert b.min() >= tiles.min() and b.max() <= tiles.max()                       # convex
    const = np.full_like(tiles, np.float32(0.3))
    assert np.abs(tl.blend_numpy(const, h, w, T, O) - np.float32(0.3)).max() < 1e-6
    assert np.array_equal(tl.blend_numpy(np.full_like(tiles, np.float32(0.75)), h, w, T, O), np.full((h, w), np.float32(0.75)))
    with pytest.raises(ValueError):
        tl.blend_numpy(tiles[:, :-1], h, w, T, O)


def test_a_pixel_may_lie_under_more_than_two_tiles_per_axis():
    """T 32, O 16 on 65 pixels: n = 4 tiles at stride 11 < T / 2 -- pixel 22 lies under three of them."""
    o = tl.axis_origins(65, 32, 16)
    assert o == [0, 11, 22, 33] and sum(1 for a in o if a <= 22 < a + 32) == 3
    tiles = np.random.default_rng(1).random((16, 32, 32)).astype(np.float32)
    assert np.abs(tl.blend_numpy(tiles, 65, 65, 32, 16) - tl.blend_numpy64(tiles, 65, 65, 32, 16)).max() < 1e-6


# ---- predict_tiled_cpu --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from models.model_2 import UNetDC
    from oracle import recipe
    torch.manual_seed(0)
    m = UNetDC(3, 1)
    recipe.perturb_bn(m.state_dict(), 5)
    return m.eval()


def test_single_tile_without_padding_is_the_plain_forward(net):
    """An image of exactly T x T is one tile at the origin, nothing folded.  With O = 0 every weight is 1, (1 p) / 1 = p: the
    result IS model(x / 255).  With O = 16 the weight w multiplies and divides again: two roundings, |fl(fl(w p) / w) - p| <=
    2 * 2^-24 p < 1.2e-7."""
    x = image(64, 64, 3, seed=3)
    with torch.no_grad():
        want = net(torch.from_numpy(x.astype(np.float32) / np.float32(255)).permute(2, 0, 1)[None])[0, 0].numpy()
    assert 0.0 < want.min() and want.max() < 1.0 and want.std() > 1e-3
    assert np.array_equal(tl.predict_tiled_cpu(net, x, 64, 0, 4), want)
    assert np.abs(tl.predict_tiled_cpu(net, x, 64, 16, 4) - want).max() <= 2.0 ** -23


def test_predict_tiled_cpu_is_blend_of_forwarded_tiles_at_any_batch(net):
    x = image(70, 100, 3, seed=4)
    tiles = torch.from_numpy(tl.gather_numpy(x, 48, 16))
    assert len(tiles) == 6
    with torch.no_grad():
        p = torch.cat([net(tiles[i:i + 1])[:, 0] for i in range(6)]).numpy()
    want = tl.blend_numpy(p, 70, 100, 48, 16)
    for batch in (4, 6):
        got = tl.predict_tiled_cpu(net, x, 48, 16, batch)
        assert got.shape == (70, 100) and got.dtype == np.float32
        assert np.abs(got - want).max() < 1e-5                                     # ATen's kernels may differ with the batch size


# ---- script -------------------------------------------------------------------------------------------------------------------
SIZES = ((100, 150), (97, 131))


def write_images(img_dir, sizes=SIZES):
    """Seeded micrograph-like PNGs: dim noise with bright discs."""
    from PIL import Image
    img_dir.mkdir()
    rng = np.random.default_rng(0)
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        img = (rng.random((h, w, 3)) * 60).astype(np.uint8)
        for _ in range(12):
            cy, cx, r = rng.integers(4, h - 4), rng.integers(4, w - 4), rng.integers(2, 9)
            img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 230
        Image.fromarray(img).save(img_dir / f"im{i}.png")


def calibrated_checkpoint(tmp_path, img_dir, radius, T, O, thresh, gain=1.0):
    """A seeded UNetDC whose head bias puts the median tile logit on the threshold (a random init is all ones at 0.3), saved as a
    checkpoint; `gain` scales out_conv.weight first (wider logits).  -> (path, model)."""
    from PIL import Image
    from models.model_2 import UNetDC
    from oracle import recipe
    from utils.data_loader import rolling_ball_correction_rgb
    torch.manual_seed(0)
    m = UNetDC(3, 1)
    recipe.perturb_bn(m.state_dict(), 5)
    m.eval()
    with torch.no_grad():
        m.out_conv.weight *= gain
        zs = []
        for f in sorted(img_dir.iterdir()):
            im = rolling_ball_correction_rgb(np.array(Image.open(f).convert("RGB")), radius)
            p = m(torch.from_numpy(tl.gather_numpy(im, T, O))).double().clamp(1e-12, 1 - 1e-12)
            zs.append(torch.log(p / (1 - p)).flatten())
        m.out_conv.bias += float(np.log(thresh / (1 - thresh))) - float(torch.cat(zs).median())
    ck = tmp_path / "ck.pth"
    torch.save(m.state_dict(), ck)
    return ck, m


def test_script_tile_on_the_cpu_path(tmp_path, monkeypatch):
    import pandas as pd
    from PIL import Image
    import quantify_droplets_batch as q
    from utils.data_loader import rolling_ball_correction_rgb
    monkeypatch.setattr(q, "DEVICE", "cpu")
    img_dir = tmp_path / "imgs"
    write_images(img_dir)
    ck, model = calibrated_checkpoint(tmp_path, img_dir, 15, 64, 16, 0.3)
    out = q.main(["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--out_dir", str(tmp_path / "out"), "--batch", "4",
                  "--prob_thresh", "0.3", "--skip_excel", "--skip_histogram", "--background_radius", "15", "--tile", "64",
                  "--tile_overlap", "16"])
    summary = pd.read_csv(out / "summary_per_image.csv")
    assert summary["filename"].tolist() == ["im0.png", "im1.png"]
    for i, (h, w) in enumerate(SIZES):
        m = np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png"))
        assert m.shape == (h, w) and set(np.unique(m)) <= {0, 255}                 # the original size
        im = rolling_ball_correction_rgb(np.array(Image.open(img_dir / f"im{i}.png").convert("RGB")), 15)
        p = tl.predict_tiled_cpu(model, im, 64, 16, 4)
        assert np.array_equal(m > 0, p > np.float32(0.3)) and 0.1 < (m > 0).mean() < 0.9
        want = q.quantify((m > 0).astype(np.uint8), 1, None)                       # the tables follow from the masks
        got = pd.read_csv(out / f"im{i}_droplets.csv", float_precision="round_trip")
        assert len(got) == len(want) > 0 and np.array_equal(got["area"].to_numpy(), want["area"].to_numpy())
        assert np.allclose(got["centroid-0"].to_numpy(), want["centroid-0"].to_numpy(), rtol=0, atol=1e-9)
        assert int(summary["droplet_count"][i]) == len(want) and int(summary["total_area_px"][i]) == int(want["area"].sum())


def test_script_tile_composes_with_the_other_stages_on_the_cpu_path(tmp_path, monkeypatch):
    """Every option works on the native-size map: split, shape, cleaning, annotation matching, sweep and density maps in one run;
    the mask is the cleaned mask of the same probabilities."""
    import pandas as pd
    from PIL import Image
    import quantify_droplets_batch as q
    from utils.data_loader import rolling_ball_correction_rgb
    from utils.droplet_clean import clean_mask
    monkeypatch.setattr(q, "DEVICE", "cpu")
    img_dir, gt_dir = tmp_path / "imgs", tmp_path / "gt"
    write_images(img_dir)
    gt_dir.mkdir()
    for i in range(2):
        im = np.array(Image.open(img_dir / f"im{i}.png").convert("RGB"))
        Image.fromarray((im[..., 0] > 125).astype(np.uint8) * 255).save(gt_dir / f"im{i}.png")
    ck, model = calibrated_checkpoint(tmp_path, img_dir, 15, 64, 16, 0.3)
    out = q.main(["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--out_dir", str(tmp_path / "out"), "--batch", "3",
                  "--prob_thresh", "0.3", "--skip_excel", "--skip_histogram", "--background_radius", "15", "--tile", "64",
                  "--tile_overlap", "16", "--split_touching", "--droplet_shape", "--fill_holes", "--prob_thresh_low", "0.25",
                  "--gt_dir", str(gt_dir), "--thresh_sweep", "10", "--sweep_objects", "0.3", "--density_maps", "--save_overlays"])
    for f in ("threshold_sweep.csv", "threshold_sweep_objects.csv", "match_per_image.csv", "mask_clean_per_image.csv",
              "density_per_image.csv", "gt_droplets.csv"):
        assert (out / f).exists(), f
    sweep = pd.read_csv(out / "threshold_sweep.csv")
    for i, (h, w) in enumerate(SIZES):
        m = np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0
        lab = np.array(Image.open(out / "predicted_masks" / f"im{i}_labels.png"))
        assert m.shape == (h, w) and lab.shape == (h, w) and (out / "overlays" / f"im{i}_overlay.png").exists()
        p = tl.predict_tiled_cpu(model, rolling_ball_correction_rgb(np.array(Image.open(img_dir / f"im{i}.png").convert("RGB")), 15),
                                 64, 16, 3)
        want = clean_mask((p > np.float32(0.3)).astype(np.uint8), (p > np.float32(0.25)).astype(np.uint8), -1)[0]
        assert np.array_equal(m, want > 0)
        assert np.array_equal(lab > 0, m)                                          # min_area 1: every mask pixel has a droplet
        got = pd.read_csv(out / f"im{i}_droplets.csv")
        assert {"perimeter", "gt_iou"} <= set(got.columns) and len(got) == lab.max()
    assert (sweep["tp"] + sweep["fp"] + sweep["fn"] + sweep["tn"] == sum(h * w for h, w in SIZES)).all()     # identity resize


def test_script_refuses_bad_tile_arguments(tmp_path):
    import quantify_droplets_batch as q
    base = ["--img_dir", str(tmp_path / "none"), "--out_dir", str(tmp_path / "out")]
    for extra, word in ((["--tile", "40"], "multiple of 16"), (["--tile", "16"], "32.."), (["--tile", "8192"], "4096"),
                        (["--tile", "64"], "overlap 64"), (["--tile", "64", "--tile_overlap", "33"], "overlap 33"),
                        (["--tile", "--tile_overlap", "-1"], "overlap -1"), (["--tile_overlap", "16"], "needs --tile"),
                        (["--tile", "--batch", "0"], "--batch")):
        with pytest.raises(SystemExit) as e:
            q.main(base + extra)
        assert word in str(e.value), (extra, e.value)
        assert not (tmp_path / "out").exists()
    a = q.build_parser().parse_args(base + ["--tile"])
    assert a.tile == 512 and q.tile_options(a) == {"T": 512, "O": 64}
    a = q.build_parser().parse_args(base + ["--tile", "64", "--tile_overlap", "0"])
    assert q.tile_options(a) == {"T": 64, "O": 0}
    assert q.tile_options(q.build_parser().parse_args(base)) is None
