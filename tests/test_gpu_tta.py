"""GPU: test-time augmentation over D4 (csrc/tta.hip, unet_dc_segmentation_amd/tta.py): the expand and mean
kernels through the C ABI against their numpy restatement (utils/tta.py), predict_tta and predict_tiled(..., tta=) against the
CPU path, and the --tta route of quantify_droplets_batch.py on the device."""
import numpy as np
import pytest
import torch

from tests.image_canaries import Canaried, canaried_like
from tests.test_gpu_tiling import BF16_PROB_BAR_EMU, BF16_PROB_BAR_F32, FP32_PROB_BAR, image, seeded_net
from tests.test_tta_cpu import fake_model
from utils import tiling as tl
from utils import tta

pytestmark = pytest.mark.gpu

# (n, C, S, N): one block; several planes of one block; 3 x 3 blocks, four channels, the flip group; 2 x 2 blocks, one flip; the
# identity alone on 4 x 4 blocks; and 12288 blocks = 3072 trips of four on a grid capped at 2048 workgroups
SHAPES = [(1, 1, 16, 8), (2, 3, 16, 8), (3, 4, 48, 4), (1, 3, 32, 2), (2, 1, 64, 1), (2, 3, 256, 8)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def expand_abi(x, N):
    """unetdc_dihedral_expand_f32 into a canaried buffer (which holds the canary pattern everywhere before the launch)."""
    from unet_dc_segmentation_amd import _lib
    n, c, s, _ = x.shape
    src, out = canaried_like(x, align=16), Canaried(n * N * c * s * s * 4, align=16)
    _lib.call("unetdc_dihedral_expand_f32", src.ptr, n, c, s, N, out.ptr, _stream())
    torch.cuda.synchronize()
    out.check("variants")
    src.check("input")
    assert np.array_equal(src.numpy(np.float32, *x.shape).view(np.uint32), x.view(np.uint32))
    return out.numpy(np.float32, n * N, c, s, s)


def mean_abi(p, N):
    from unet_dc_segmentation_amd import _lib
    s, n = p.shape[-1], p.shape[0] // N
    src, out = canaried_like(p, align=16), Canaried(n * s * s * 4, align=16)
    _lib.call("unetdc_dihedral_mean_f32", src.ptr, n, s, N, out.ptr, _stream())
    torch.cuda.synchronize()
    out.check("mean")
    src.check("items")
    return out.numpy(np.float32, n, s, s)


@pytest.mark.parametrize("n,c,s,N", SHAPES)
def test_expand_bit_exact(n, c, s, N):
    x = np.random.default_rng(s + N).permutation(n * c * s * s).astype(np.float32).reshape(n, c, s, s)     # distinct, exact below 2^24
    got = expand_abi(x, N)
    assert np.array_equal(got.view(np.uint32), tta.expand_numpy(x, N).view(np.uint32))


@pytest.mark.parametrize("n,c,s,N", SHAPES)
def test_mean_bit_exact_round_trip_and_determinism(n, c, s, N):
    n = n * c                                                                     # the mean has no channels: as many planes
    p = np.random.default_rng(s * N).random((n * N, s, s), dtype=np.float32)
    a, b = mean_abi(p, N), mean_abi(p, N)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))                    # two runs, the same bytes
    assert np.array_equal(a.view(np.uint32), tta.mean_numpy(p, N).view(np.uint32))  # the same fp32 operations
    err = float(np.abs(a - tta.mean_numpy64(p, N)).max())
    print(f"[mean n{n} S{s} N{N}] max |device - fp64| = {err:.3e}")
    assert err <= (N - 1) * 2.0 ** -24
    x = (np.random.default_rng(n).integers(0, 256, (n, 1, s, s)) / 256).astype(np.float32)
    back = mean_abi(expand_abi(x, N)[:, 0], N)                                    # k / 256: no fp32 operation rounds
    assert np.array_equal(back.view(np.uint32), x[:, 0].view(np.uint32))


def test_mean_past_the_grid_cap():
    """34 images of 256 x 256, N = 2: 8704 output blocks = 2176 trips of four on a grid capped at 2048 workgroups."""
    from unet_dc_segmentation_amd.tta import dihedral_mean
    p = np.random.default_rng(3).random((68, 256, 256), dtype=np.float32)
    got = dihedral_mean(torch.from_numpy(p).cuda(), 2).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), tta.mean_numpy(p, 2).view(np.uint32))


def test_wrappers_match_the_abi_and_check_their_arguments():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.tta import dihedral_expand, dihedral_mean
    x = np.random.default_rng(1).random((2, 3, 32, 32), dtype=np.float32)
    d = torch.from_numpy(x).cuda()
    e = dihedral_expand(d, 4)
    assert np.array_equal(e.cpu().numpy().view(np.uint32), tta.expand_numpy(x, 4).view(np.uint32))
    out = torch.empty(8, 3, 32, 32, device="cuda")
    assert dihedral_expand(d, 4, out=out) is out and torch.equal(out, e)
    p = e[:, 0].contiguous()
    m = dihedral_mean(p, 4)
    assert np.array_equal(m.cpu().numpy().view(np.uint32), tta.mean_numpy(p.cpu().numpy(), 4).view(np.uint32))
    out = torch.empty(2, 32, 32, device="cuda")
    assert dihedral_mean(p, 4, out=out) is out and torch.equal(out, m)
    for bad in (lambda: dihedral_expand(d, 3), lambda: dihedral_expand(d, 16), lambda: dihedral_expand(d.double(), 4),
                lambda: dihedral_expand(torch.from_numpy(x), 4), lambda: dihedral_expand(d[0], 4),
                lambda: dihedral_expand(d[..., :16], 4), lambda: dihedral_expand(torch.zeros(1, 3, 24, 24, device="cuda"), 4),
                lambda: dihedral_expand(torch.zeros(1, 5, 16, 16, device="cuda"), 4),
                lambda: dihedral_expand(d, 4, out=torch.empty(8, 3, 32, 32)), lambda: dihedral_expand(d, 4, out=out),
                lambda: dihedral_expand(d, 4, out=torch.empty(8, 3, 32, 32, device="cuda", dtype=torch.float64)),
                lambda: dihedral_expand(d, 4, out=torch.empty(8, 3, 32, 64, device="cuda")[..., :32]),
                lambda: dihedral_mean(p, 3), lambda: dihedral_mean(p[:7], 4), lambda: dihedral_mean(e, 4),
                lambda: dihedral_mean(p.cpu(), 4), lambda: dihedral_mean(p.half(), 4),
                lambda: dihedral_mean(p, 4, out=torch.empty(8, 32, 32, device="cuda")),
                lambda: dihedral_mean(p, 4, out=torch.empty(2, 32, 32))):
        with pytest.raises(_lib.UnetdcError):
            bad()


# ---- predict_tta ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,batch", [(8, 3), (4, 8), (2, 12), (1, 2)])
def test_predict_tta_with_the_fake_model_is_the_cpu_path_bit_for_bit(N, batch):
    """The fake model (tests/test_tta_cpu.py) is exact on either device, so expand, chunk rule and mean are all that can differ."""
    from unet_dc_segmentation_amd.tta import predict_tta
    x = torch.from_numpy(np.random.default_rng(N + batch).random((5, 3, 32, 32), dtype=np.float32))
    want = tta.predict_tta_cpu(fake_model, x, N, batch).numpy()
    got = predict_tta(fake_model, x.cuda(), N, batch)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (5, 1, 32, 32)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def own_variants(net, x, N, batch):
    """The HIP module's outputs on the items of dihedral_expand, in the slices predict_tta forwards (groups of max(1, batch // N)
    images, `batch` items per forward)."""
    from unet_dc_segmentation_amd.tta import dihedral_expand
    out = []
    with torch.no_grad():
        for b0, g in tta.groups(len(x), N, batch):
            items = dihedral_expand(x[b0:b0 + g], N)
            out += [net(items[i:i + batch])[:, 0].float().clone() for i in range(0, g * N, batch)]
    return torch.cat(out).cpu().numpy()


def test_predict_tta_fp32_against_its_own_variants_and_the_cpu_path():
    """3 images of 48 x 48, N = 8, 4 items per forward: groups of one image, two forwards each, ONE engine shape."""
    import copy
    from unet_dc_segmentation_amd.tta import predict_tta
    cpu_net = seeded_net()
    net = copy.deepcopy(cpu_net).cuda().eval()
    x = torch.from_numpy(np.random.default_rng(7).random((3, 3, 48, 48), dtype=np.float32))
    d = x.cuda()
    got = predict_tta(net, d, 8, 4)
    assert tuple(got.shape) == (3, 1, 48, 48) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    assert len(net._engines) <= 2 and sum(len(v) for v in net._engines.values()) <= net.MAX_ENGINES
    e_own = float(np.abs(got[:, 0] - tta.mean_numpy64(own_variants(net, d, 8, 4), 8)).max())
    ref = tta.predict_tta_cpu(cpu_net, x, 8, 4).numpy()
    e_cpu = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"[predict_tta] max |device - fp64 mean of its own variants| = {e_own:.3e}, max |device - CPU path| = {e_cpu:.3e}")
    assert ref.std() > 1e-3                                                        # the map is not flat
    assert e_own < 1e-6
    assert e_cpu < FP32_PROB_BAR                                                   # the mean is convex: the bar passes through
    again = predict_tta(net, d, 8, 4).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_predict_tta_bf16_against_both_oracles():
    """The shapes of the fp32 test with set_compute_dtype("bf16"): what quantify_droplets_batch.py --tta --dtype bf16 runs.  The
    comparison maps are the fp64 means of the CPU oracle's outputs on the expand_numpy items, once with bf16 storage emulated and
    once in plain fp32.  Measured on MI355X: 3.1e-4 against the emulation, 2.8e-4 against fp32, 6.0e-8 against the fp64 mean of the
    device's own variant outputs."""
    import copy
    from oracle import unetdc_torch_cpu as otc
    from unet_dc_segmentation_amd.tta import predict_tta
    cpu_net = seeded_net()
    sd = {k: v.detach().clone() for k, v in cpu_net.state_dict().items()}
    net = copy.deepcopy(cpu_net).cuda().eval()
    net.set_compute_dtype("bf16")
    x = np.random.default_rng(7).random((3, 3, 48, 48), dtype=np.float32)
    d = torch.from_numpy(x).cuda()
    got = predict_tta(net, d, 8, 4)
    assert tuple(got.shape) == (3, 1, 48, 48) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    assert len(net._engines) <= 2 and sum(len(v) for v in net._engines.values()) <= net.MAX_ENGINES
    e_own = float(np.abs(got[:, 0] - tta.mean_numpy64(own_variants(net, d, 8, 4), 8)).max())
    items = torch.from_numpy(tta.expand_numpy(x, 8))
    maps = {}
    with torch.no_grad():                                                          # eval mode: an item's output does not depend on its chunk
        for tag, emu in (("emu", True), ("f32", False)):
            p = otc.unet_forward(items, sd, dict(cpu_net.DILATIONS), train=False, emulate_bf16=emu)[:, 0].numpy()
            maps[tag] = tta.mean_numpy64(p, 8)
    e_emu = float(np.abs(got[:, 0].astype(np.float64) - maps["emu"]).max())
    e_f32 = float(np.abs(got[:, 0].astype(np.float64) - maps["f32"]).max())
    print(f"[predict_tta bf16] max |device - fp64 mean of its own variants| = {e_own:.3e}, max |device - bf16-storage oracle| = "
          f"{e_emu:.3e}, max |device - fp32 oracle| = {e_f32:.3e}")
    assert maps["f32"].std() > 1e-3
    assert e_own < 1e-6
    assert e_emu < BF16_PROB_BAR_EMU
    assert e_f32 < BF16_PROB_BAR_F32
    again = predict_tta(net, d, 8, 4).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_predict_tiled_with_tta_against_the_cpu_path():
    """80 x 112, T 48, O 16, 4 items per forward, N = 8: 2 x 3 tiles, each a group of its own of two forwards."""
    import copy
    from unet_dc_segmentation_amd.tiling import predict_tiled
    h, w, T, O, batch = 80, 112, 48, 16, 4
    img = image(h, w, 3, seed=11)
    cpu_net = seeded_net()
    net = copy.deepcopy(cpu_net).cuda().eval()
    d = torch.from_numpy(img).cuda()
    got = predict_tiled(net, d, T, O, batch, tta=8)
    assert got.shape == (h, w) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    assert len(net._engines) <= 2
    ref = tl.predict_tiled_cpu(cpu_net, img, T, O, batch, tta=8)
    e_cpu = float(np.abs(got.astype(np.float64) - ref).max())
    plain = predict_tiled(net, d, T, O, batch).cpu().numpy()
    print(f"[predict_tiled tta 8] max |device - CPU path| = {e_cpu:.3e}, max |with - without tta| = {np.abs(got - plain).max():.3e}")
    assert ref.std() > 1e-3 and e_cpu < FP32_PROB_BAR
    assert np.abs(got - plain).max() > 10 * FP32_PROB_BAR                          # the variants did run
    assert np.array_equal(predict_tiled(net, d, T, O, batch, tta=1).cpu().numpy().view(np.uint32), plain.view(np.uint32))


# ---- script -------------------------------------------------------------------------------------------------------------------
def guarded_masks_agree(m, p, tag):
    """The device mask against the CPU rule's probabilities: equal on every pixel whose probability lies more than the fp32 bar
    from the threshold, and at most 5 % of the pixels lie inside that band."""
    p = p.astype(np.float64)
    guard = np.abs(p - 0.3) > FP32_PROB_BAR
    excluded = 1.0 - float(guard.mean())
    print(f"[{tag}] excluded {excluded:.4f} of the pixels, mask differs on {int((m != (p > 0.3)).sum())} pixels")
    assert m.shape == p.shape and 0.1 < m.mean() < 0.9
    assert excluded <= 0.05
    assert np.array_equal(m[guard], (p > 0.3)[guard])


def test_script_tile_tta_on_the_device(tmp_path):
    """quantify_droplets_batch.main --tile 64 --tile_overlap 16 --tta 8 --batch 4 on the device against the same entry point's CPU
    rule (predict_tiled_cpu(..., tta=8)).  The checkpoint is widened by gain = 4.0: averaging narrows the logits, and at gain 1.0
    the CPU reference alone would keep 7.3 % / 7.4 % of the pixels inside the band (2.1 % / 1.8 % at 4.0)."""
    import pandas as pd
    from PIL import Image
    import quantify_droplets_batch as q
    from tests.test_tiling_cpu import SIZES, calibrated_checkpoint, write_images
    from utils.data_loader import rolling_ball_correction_rgb
    assert q.DEVICE == "cuda"
    img_dir = tmp_path / "imgs"
    write_images(img_dir)
    ck, model = calibrated_checkpoint(tmp_path, img_dir, 15, 64, 16, 0.3, gain=4.0)
    out = q.main(["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--batch", "4", "--prob_thresh", "0.3", "--skip_excel",
                  "--skip_histogram", "--background_radius", "15", "--tile", "64", "--tile_overlap", "16", "--tta", "8",
                  "--out_dir", str(tmp_path / "gpu")])
    for i, (h, w) in enumerate(SIZES):
        m = np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0
        im = rolling_ball_correction_rgb(np.array(Image.open(img_dir / f"im{i}.png").convert("RGB")), 15)
        guarded_masks_agree(m, tl.predict_tiled_cpu(model, im, 64, 16, 4, tta=8), f"script --tile --tta 8 im{i}")
        got = pd.read_csv(out / f"im{i}_droplets.csv")
        want = q.quantify(m.astype(np.uint8), 1, None)                             # the tables follow from the masks
        assert len(got) == len(want) and int(got["area"].sum()) == int(want["area"].sum())


def test_script_squash_tta_on_the_device(tmp_path, monkeypatch):
    """The route without --tile, --tta 4 --batch 4: run_batch forwards the network-size inputs through predict_tta.  Two images
    of the network's size (lowered to 128 x 128, so that the CPU reference takes a second) make every resize the identity; the
    device preprocessing is bit-equal to the host's (test_gpu_preprocess.py), so the reference is predict_tta_cpu on the same
    inputs.  The checkpoint's gain was chosen on the CPU: at gain 4.0 the reference alone keeps 1.2 % / 1.3 % of the pixels inside
    the band (5.7 % / 5.5 % at gain 1.0, over the cap)."""
    from PIL import Image
    import quantify_droplets_batch as q
    from tests.test_tiling_cpu import calibrated_checkpoint, write_images
    assert q.DEVICE == "cuda"
    monkeypatch.setattr(q, "IMG_SIZE", 128)
    img_dir = tmp_path / "imgs"
    write_images(img_dir, sizes=((128, 128), (128, 128)))
    ck, model = calibrated_checkpoint(tmp_path, img_dir, 15, 128, 0, 0.3, gain=4.0)     # one tile = the whole corrected image
    out = q.main(["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--batch", "4", "--prob_thresh", "0.3", "--skip_excel",
                  "--skip_histogram", "--background_radius", "15", "--tta", "4", "--out_dir", str(tmp_path / "gpu")])
    xs = torch.stack([q.preprocess(img_dir / f"im{i}.png", 15)[0] for i in range(2)]).cpu()
    p = tta.predict_tta_cpu(model, xs, 4, 4)[:, 0].numpy()
    for i in range(2):
        m = np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0
        guarded_masks_agree(m, p[i], f"script --tta 4 im{i}")
