"""CPU: test-time augmentation over D4 -- the variants, the numpy restatement of the expand and mean
kernels (utils/tta.py), predict_tta_cpu, the tta argument of predict_tiled_cpu, the --tta route of quantify_droplets_batch.py
and of train_DC_focal.py on the CPU path, and the refusals of the two C-ABI entry points (host code: no device needed)."""
import itertools

import numpy as np
import pytest
import torch

from utils import tiling as tl
from utils import tta

D4 = range(8)


def plane(S, seed=0):
    """Distinct values: any index error shows."""
    return np.random.default_rng(seed).permutation(S * S).astype(np.float32).reshape(S, S)


def restated(p, v):
    """The definition, written out: hflip = v & 4, k = v & 3, flip first."""
    return np.rot90(p[:, ::-1] if v & 4 else p, v & 3)


# ---- variants -------------------------------------------------------------------------------------------------------------------
def test_lists_and_limits():
    assert tta.TTA_SIZES == (1, 2, 4, 8)
    assert [list(tta.variants(N)) for N in tta.TTA_SIZES] == [[0], [0, 4], [0, 4, 2, 6], list(range(8))]
    for bad in (0, 3, 5, 16, -8, 2.5, True):
        with pytest.raises(ValueError):
            tta.check_tta(bad)
    assert tta.check_tta(np.int64(4)) == 4
    for shape in ((1, 3, 16, 32), (1, 3, 24, 24), (3, 16, 16), (1, 1, 8, 8)):
        with pytest.raises(ValueError):
            tta.expand_numpy(np.zeros(shape, np.float32), 2)
    with pytest.raises(ValueError):
        tta.mean_numpy(np.zeros((3, 16, 16), np.float32), 2)              # 3 items are no multiple of 2


@pytest.mark.parametrize("S", (16, 48))
def test_expand_is_rot90_after_the_flip(S):
    x = np.stack([np.stack([plane(S, 3 * b + c) for c in range(3)]) for b in range(2)])
    for N in tta.TTA_SIZES:
        out = tta.expand_numpy(x, N)
        assert out.shape == (2 * N, 3, S, S) and out.dtype == np.float32
        for b, (i, v), c in itertools.product(range(2), enumerate(tta.variants(N)), range(3)):
            assert np.array_equal(out[b * N + i, c], restated(x[b, c], v)), (N, b, i, c)
    assert np.array_equal(tta.expand_numpy(x, 1), x)


def test_variant_follows_the_training_augmentation():
    """The order of tests/augment_ref.py::augment_with_params: hflip, (vflip,) then rot90."""
    from tests.augment_ref import augment_with_params
    img = plane(16, 5)[..., None].repeat(3, 2)
    for v in D4:
        got = augment_with_params(img, img[..., 0], dict(hflip=bool(v & 4), vflip=False, k=v & 3, bc=False, alpha=1.0, beta=0.0,
                                                         elastic=False))[0]
        assert np.array_equal(np.asarray(got)[..., 0], restated(img[..., 0], v)), v


def test_inverse_after_forward_is_the_identity():
    p = plane(32, 1)
    for v in D4:
        assert np.array_equal(tta.variant_inverse(tta.variant(p, v), v), p), v
        assert np.array_equal(tta.variant(tta.variant_inverse(p, v), v), p), v
        assert np.array_equal(tta.variant(p, v), restated(p, v))


def test_the_list_of_four_is_the_flip_group():
    p = plane(16, 2)
    got = [tta.variant(p, v) for v in tta.variants(4)]
    want = [p, np.fliplr(p), np.rot90(p, 2), np.flipud(p)]
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for a, b in itertools.product(tta.variants(4), repeat=2):              # closed under composition
        ab = tta.variant(tta.variant(p, a), b)
        assert sum(np.array_equal(ab, g) for g in got) == 1, (a, b)
    assert sum(np.array_equal(tta.variant(tta.variant(p, 4), 1), g) for g in got) == 0        # a quarter turn leaves it
    assert len({tta.variant(p, v).tobytes() for v in D4}) == 8             # all of D4: eight different planes


# ---- mean ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", tta.TTA_SIZES)
def test_mean_of_the_expansion_is_the_input_bit_for_bit(N):
    """Planes of k / 256: every partial sum of at most 8 such values is a multiple of 2^-8 below 8, exact in fp32, and so is the
    division by a power of two."""
    x = (np.random.default_rng(N).integers(0, 256, (3, 1, 48, 48)) / 256).astype(np.float32)
    got = tta.mean_numpy(tta.expand_numpy(x, N)[:, 0], N)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x[:, 0].view(np.uint32))


@pytest.mark.parametrize("N", tta.TTA_SIZES)
def test_mean_against_fp64_and_its_own_definition(N):
    """N - 1 adds of values in [0, 1], each within half an ulp of a partial sum below 8 (2^-22 / 2 ... the sum of the N - 1
    rounding errors is below (N - 1) 2^-22 before the division by N >= 2 ... ) -- the issue's bound: (N - 1) 2^-24 after it."""
    p = np.random.default_rng(10 + N).random((2 * N, 32, 32), dtype=np.float32)
    a, b = tta.mean_numpy(p, N), tta.mean_numpy64(p, N)
    assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape == (2, 32, 32)
    assert np.abs(a - b).max() <= (N - 1) * 2.0 ** -24
    for img in range(2):                                                   # the rule, written out per pixel order
        acc = None
        for i, v in enumerate(tta.variants(N)):
            q = np.rot90(p[img * N + i], -(v & 3))
            q = q[:, ::-1] if v & 4 else q
            acc = q.astype(np.float32) if acc is None else acc + q
        assert np.array_equal(a[img], acc / np.float32(N))
    if N == 1:
        assert np.array_equal(a.view(np.uint32), p.view(np.uint32))


# ---- predict_tta_cpu ------------------------------------------------------------------------------------------------------------
def fake_model(x):
    """Per item, asymmetric under every flip and turn, and exact: products with powers of two and two adds of values in [0, 1],
    so that a forward gives the same bits whatever the batch it runs in (and on whatever device)."""
    return (0.5 * x[:, 0:1] + 0.25 * torch.roll(x[:, 1:2], 1, -1) + 0.125 * torch.roll(x[:, 2:3], 1, -2)).clamp(0.0, 1.0)


def by_hand(model, x, N):
    out = []
    for img in x.numpy():
        acc = None
        for v in tta.variants(N):
            p = model(torch.from_numpy(np.ascontiguousarray(restated_chw(img, v)))[None])[0, 0].numpy()
            q = np.rot90(p, -(v & 3))
            q = q[:, ::-1] if v & 4 else q
            acc = q.copy() if acc is None else acc + q
        out.append(acc / np.float32(N))
    return np.stack(out)[:, None]


def restated_chw(img, v):
    return np.stack([restated(c, v) for c in img])


@pytest.mark.parametrize("N", tta.TTA_SIZES)
def test_predict_tta_cpu_is_the_hand_written_loop_at_any_batch(N):
    x = torch.from_numpy(np.random.default_rng(N).random((5, 3, 32, 32), dtype=np.float32))
    want = by_hand(fake_model, x, N)
    assert want.std() > 0.05
    for batch in (1, 3, 8, 12):
        got = tta.predict_tta_cpu(fake_model, x, N, batch)
        assert got.shape == (5, 1, 32, 32) and got.dtype == torch.float32
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), batch
    assert tta.groups(5, N, 8) == [(b0, min(max(1, 8 // N), 5 - b0)) for b0 in range(0, 5, max(1, 8 // N))]


def test_fake_model_alone_is_not_equivariant():
    x = torch.from_numpy(np.random.default_rng(0).random((1, 3, 32, 32), dtype=np.float32))
    for g in range(1, 8):
        gx = torch.from_numpy(np.ascontiguousarray(tta.variant(x.numpy(), g)))
        assert np.abs(fake_model(gx).numpy() - tta.variant(fake_model(x).numpy(), g)).max() > 0.05, g


@pytest.mark.parametrize("N", (2, 4, 8))
def test_equivariance_defect(N):
    """F(g x) against g F(x) for every g of the averaged subgroup (all of D4 at N = 8; a g outside the subgroup permutes its
    cosets and F is not equivariant under it).  Both sides are fp32 means of the SAME N exact model outputs in different orders,
    each within (N - 1) 2^-24 of the exact mean: a defect of at most 2 (N - 1) 2^-24."""
    x = torch.from_numpy(np.random.default_rng(20 + N).random((2, 3, 32, 32), dtype=np.float32))
    fx = tta.predict_tta_cpu(fake_model, x, N, 8).numpy()
    for g in tta.variants(N):
        gx = torch.from_numpy(np.ascontiguousarray(tta.variant(x.numpy(), g)))
        defect = np.abs(tta.predict_tta_cpu(fake_model, gx, N, 8).numpy().astype(np.float64) - tta.variant(fx, g)).max()
        assert defect <= 2 * (N - 1) * 2.0 ** -24, (g, defect)


# ---- predict_tiled_cpu ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from models.model_2 import UNetDC
    from oracle import recipe
    torch.manual_seed(0)
    m = UNetDC(3, 1)
    recipe.perturb_bn(m.state_dict(), 5)
    return m.eval()


def test_predict_tiled_cpu_without_tta_is_unchanged(net):
    """tta=1 (and no tta argument) is the code of before: the blend of the tiles forwarded in chunks of `batch`."""
    x = np.random.default_rng(4).integers(0, 256, (70, 100, 3)).astype(np.uint8)
    tiles = torch.from_numpy(tl.gather_numpy(x, 48, 16))
    with torch.no_grad():
        p = torch.cat([net(tiles[i:i + 4])[:, 0] for i in range(0, len(tiles), 4)]).numpy()
    want = tl.blend_numpy(p, 70, 100, 48, 16)
    for got in (tl.predict_tiled_cpu(net, x, 48, 16, 4), tl.predict_tiled_cpu(net, x, 48, 16, 4, tta=1)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        tl.predict_tiled_cpu(net, x, 48, 16, 4, tta=3)


def test_predict_tiled_cpu_with_tta_is_the_blend_of_the_tile_means(net):
    x = np.random.default_rng(5).integers(0, 256, (50, 70, 3)).astype(np.uint8)
    tiles = torch.from_numpy(tl.gather_numpy(x, 48, 16))
    assert len(tiles) == 4
    want = tl.blend_numpy(tta.predict_tta_cpu(net, tiles, 2, 4)[:, 0].numpy(), 50, 70, 48, 16)
    got = tl.predict_tiled_cpu(net, x, 48, 16, 4, tta=2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(got - tl.predict_tiled_cpu(net, x, 48, 16, 4)).max() > 1e-4      # the network is not flip-equivariant


# ---- scripts --------------------------------------------------------------------------------------------------------------------
def test_script_tile_tta_on_the_cpu_path(tmp_path, monkeypatch):
    import pandas as pd
    from PIL import Image
    import quantify_droplets_batch as q
    from tests.test_tiling_cpu import SIZES, calibrated_checkpoint, write_images
    from utils.data_loader import rolling_ball_correction_rgb
    monkeypatch.setattr(q, "DEVICE", "cpu")
    img_dir = tmp_path / "imgs"
    write_images(img_dir)
    ck, model = calibrated_checkpoint(tmp_path, img_dir, 15, 64, 16, 0.3, gain=4.0)
    args = ["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--batch", "4", "--prob_thresh", "0.3", "--skip_excel",
            "--skip_histogram", "--background_radius", "15", "--tile", "64", "--tile_overlap", "16"]
    out = q.main(args + ["--out_dir", str(tmp_path / "tta"), "--tta", "8"])
    plain = q.main(args + ["--out_dir", str(tmp_path / "plain")])
    summary = pd.read_csv(out / "summary_per_image.csv")
    for i, (h, w) in enumerate(SIZES):
        m = np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0
        im = rolling_ball_correction_rgb(np.array(Image.open(img_dir / f"im{i}.png").convert("RGB")), 15)
        p = tl.predict_tiled_cpu(model, im, 64, 16, 4, tta=8)
        assert m.shape == (h, w) and np.array_equal(m, p > np.float32(0.3)) and 0.1 < m.mean() < 0.9
        m0 = np.array(Image.open(plain / "predicted_masks" / f"im{i}_pred.png")) > 0
        share = float((m != m0).mean())
        print(f"[script --tile --tta 8 im{i}] the mask differs from the run without --tta on {share:.3f} of the pixels")
        assert share > 0.05                                                # about 0.37 at this checkpoint
        want = q.quantify(m.astype(np.uint8), 1, None)                     # the tables follow from the masks
        got = pd.read_csv(out / f"im{i}_droplets.csv", float_precision="round_trip")
        assert len(got) == len(want) > 0 and np.array_equal(got["area"].to_numpy(), want["area"].to_numpy())
        assert int(summary["droplet_count"][i]) == len(want) and int(summary["total_area_px"][i]) == int(want["area"].sum())


def test_script_squash_tta_on_the_cpu_path(tmp_path, monkeypatch):
    """Without --tile: run_batch forwards the 512 x 512 squash through predict_tta_cpu (IMG_SIZE lowered to 64 to keep the
    CPU forwards small)."""
    from PIL import Image
    import quantify_droplets_batch as q
    from tests.test_tiling_cpu import SIZES, calibrated_checkpoint, write_images
    monkeypatch.setattr(q, "DEVICE", "cpu")
    monkeypatch.setattr(q, "IMG_SIZE", 64)
    img_dir = tmp_path / "imgs"
    write_images(img_dir)
    ck, model = calibrated_checkpoint(tmp_path, img_dir, 15, 64, 16, 0.3, gain=4.0)
    out = q.main(["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--batch", "2", "--prob_thresh", "0.3", "--skip_excel",
                  "--skip_histogram", "--background_radius", "15", "--out_dir", str(tmp_path / "out"), "--tta", "2"])
    x = torch.stack([q.preprocess(img_dir / f"im{i}.png", 15)[0] for i in range(2)])
    p = tta.predict_tta_cpu(model, x, 2, 2)[:, 0]
    for i, (h, w) in enumerate(SIZES):
        m = np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0
        want = q.resize_mask_like_reference((p[i] > 0.3).to(torch.uint8).numpy(), w, h) > 0
        assert m.shape == (h, w) and np.array_equal(m, want) and 0.02 < m.mean() < 0.98


def test_script_refuses_bad_tta_values(tmp_path):
    import quantify_droplets_batch as q
    base = ["--img_dir", str(tmp_path / "none"), "--out_dir", str(tmp_path / "out")]
    for n in ("0", "3", "16"):
        for route in ([], ["--tile"]):
            with pytest.raises(SystemExit) as e:
                q.main(base + route + ["--tta", n])
            assert "--tta" in str(e.value) and n in str(e.value), e.value
            assert not (tmp_path / "out").exists()
    with pytest.raises(SystemExit) as e:
        q.main(base + ["--tta", "--batch", "0"])
    assert "--batch" in str(e.value)
    parse = q.build_parser().parse_args
    assert parse(base + ["--tta"]).tta == 8 and q.tta_options(parse(base + ["--tta", "--batch", "4"])) == {"N": 8, "batch": 4}
    assert q.tta_options(parse(base)) is None and q.tta_options(parse(base + ["--tta", "1"])) is None


TRAIN_ARGS = ["--synthetic", "--synthetic_len", "10", "--img_size", "32", "--batch", "2", "--epochs", "1", "--steps", "1",
              "--workers", "0", "--in_channels", "1", "--device", "cpu"]


def test_train_tta_applies_to_the_final_evaluations_only(tmp_path, monkeypatch, capsys):
    """--tta 4 on the CPU path: the training step and the validation pass forward 2 images at a time as before; the test
    evaluation and the calibration forward the 4 variants of their images, --batch items at a time."""
    import train_DC_focal as t
    seen = []
    real = t.predict_eval
    monkeypatch.setattr(t, "predict_eval", lambda model, images, n, batch: (seen.append((tuple(images.shape), n, batch)),
                                                                           real(model, images, n, batch))[1])
    ck = str(tmp_path / "ck.pth")
    h = t.main(TRAIN_ARGS + ["--ckpt_path", ck, "--tta", "4", "--calibrate_thresh", "10"])
    assert h.tta == 4 and h.test is not None and h.calibration["hist"].sum() == 2 * 32 * 32
    assert seen == [((2, 1, 32, 32), 4, 2)] * 2                            # one test batch, one calibration batch
    assert "--tta 4" in capsys.readouterr().out
    plain = t.main(TRAIN_ARGS + ["--ckpt_path", ck])
    assert plain.tta == 1 and t.build_parser().parse_args(["--tta"]).tta == 8
    for bad in ("0", "3", "16"):
        with pytest.raises(SystemExit) as e:
            t.main(TRAIN_ARGS + ["--ckpt_path", ck, "--tta", bad])
        assert "--tta" in str(e.value)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments_without_a_device():
    """The checks are host code in front of the launch: a refused call touches no pointer, so made-up addresses do."""
    from unet_dc_segmentation_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    X, OUT = 0x10000000, 0x20000000

    def expand(**kw):
        a = dict(x=X, n=2, c=3, s=32, nvar=4, out=OUT)
        a.update(kw)
        return lib.unetdc_dihedral_expand_f32(a["x"], a["n"], a["c"], a["s"], a["nvar"], a["out"], None)

    def mean(**kw):
        a = dict(p=X, n=2, s=32, nvar=4, out=OUT)
        a.update(kw)
        return lib.unetdc_dihedral_mean_f32(a["p"], a["n"], a["s"], a["nvar"], a["out"], None)

    common = [(dict(out=None), "null"), (dict(s=0), "limits"), (dict(s=8), "limits"), (dict(s=40), "limits"), (dict(s=4112), "limits"),
              (dict(s=-16), "limits"), (dict(n=0), "geometry"), (dict(n=4097), "geometry"), (dict(nvar=0), "variants"),
              (dict(nvar=3), "variants"), (dict(nvar=16), "variants"), (dict(nvar=-8), "variants"), (dict(out=OUT + 4), "aligned"),
              (dict(out=X), "overlap"), (dict(out=X + 16), "overlap")]
    in_bytes = 2 * 3 * 32 * 32 * 4
    for kw, word in common + [(dict(x=None), "null"), (dict(c=0), "geometry"), (dict(c=5), "geometry"), (dict(x=X + 8), "aligned"),
                              (dict(out=X + in_bytes - 16), "overlap"), (dict(out=X - 4 * in_bytes + 16), "overlap")]:
        assert expand(**kw) == -1 and word.encode() in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    out_bytes = 2 * 32 * 32 * 4
    for kw, word in common + [(dict(p=None), "null"), (dict(p=X + 8), "aligned"), (dict(out=X + 4 * out_bytes - 16), "overlap"),
                              (dict(out=X - out_bytes + 16), "overlap")]:
        assert mean(**kw) == -1 and word.encode() in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
