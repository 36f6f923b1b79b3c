"""GPU: tiled inference at native resolution (csrc/tile.hip, unet_dc_segmentation_amd/tiling.py): the
gather and blend kernels through the C ABI against their numpy restatement (utils/tiling.py), predict_tiled against the CPU
path, and the --tile route of quantify_droplets_batch.py on the device."""
import numpy as np
import pytest
import torch

from tests.image_canaries import Canaried, canaried_like
from utils import tiling as tl

pytestmark = pytest.mark.gpu

FP32_PROB_BAR = 2.5e-4 + 1e-6      # the project's fp32 bar of 1e-3 before the sigmoid, whose slope is at most 1/4; the blend is
#                                    convex, so it passes the bar on and adds its own 1e-6 (test_tiling_cpu.py)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def image(h, w, c, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c)).astype(np.uint8)


def plan_dev(h, w, T, O):
    yo, xo = tl.tile_plan(h, w, T, O)
    return torch.tensor(yo, dtype=torch.int32, device="cuda"), torch.tensor(xo, dtype=torch.int32, device="cuda")


def gather_abi(img, T, O, chunks):
    """unetdc_tile_gather_u8_to_chw_f32 over the (t0, count) chunks, each into its slice of ONE canaried [n, C, T, T] buffer.
    O None: one tile at the origin (a tile size below the plan's limit of 32, which the kernel takes)."""
    from unet_dc_segmentation_amd import _lib
    h, w, c = img.shape
    yo, xo = plan_dev(h, w, T, O) if O is not None else (torch.zeros(1, dtype=torch.int32, device="cuda"),) * 2
    n = len(yo) * len(xo)
    src, out = canaried_like(img, align=16), Canaried(n * c * T * T * 4, align=16)
    for t0, count in chunks(n):
        _lib.call("unetdc_tile_gather_u8_to_chw_f32", src.ptr, h, w, c, out.ptr + t0 * c * T * T * 4, T, yo.data_ptr(), len(yo),
                  xo.data_ptr(), len(xo), t0, count, _stream())
    torch.cuda.synchronize()
    out.check("tile buffer")
    src.check("image")
    assert np.array_equal(src.numpy(np.uint8, h, w, c), img)
    return out.numpy(np.float32, n, c, T, T)


def one_shot(n):
    return [(0, n)]


def by(k):
    return lambda n: [(t0, min(k, n - t0)) for t0 in range(0, n, k)]


GATHER = [(37, 53, 3, 32, 8),      # ragged, 2 x 2 tiles
          (20, 70, 3, 32, 8),      # one axis shorter than the tile: a single reflection
          (5, 9, 1, 16, None),     # several reflections on both axes, one channel; one tile of 16 at the origin
          (5, 9, 1, 32, 0),        # ... and more of them through the plan
          (1, 1, 3, 32, 8),        # a side of one pixel
          (33, 100, 4, 32, 16)]    # four channels, 2 x 6 tiles, up to three tiles over a pixel


@pytest.mark.parametrize("h,w,c,T,O", GATHER)
def test_gather_bit_exact(h, w, c, T, O):
    img = image(h, w, c, seed=h + w)
    want = tl.gather_numpy(img, T, O) if O is not None else tl.gather_at_numpy(img, T, [0], [0])
    got = gather_abi(img, T, O, one_shot)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("k", (1, 4))
def test_gather_in_chunks_equals_one_shot(k):
    h, w, c, T, O = 37, 124, 3, 32, 8          # 2 x 5 = 10 tiles: chunks of 4 are 4 + 4 + 2 and start inside a row of the plan
    img = image(h, w, c, seed=k)
    want = tl.gather_numpy(img, T, O)
    assert len(want) == 10
    got = gather_abi(img, T, O, by(k))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_gather_past_the_grid_cap():
    """A micrograph's plan, 3 x 3 tiles of 512: 589824 groups of four pixels on a grid capped at 2048 x 256 threads."""
    img = image(1040, 1388, 1, seed=2)
    want = tl.gather_numpy(img, 512, 64)
    assert len(want) == 9
    got = gather_abi(img, 512, 64, one_shot)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_wrapper_gather_matches_abi_and_checks_its_arguments():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.tiling import tile_gather
    img = image(37, 53, 3, seed=9)
    want = tl.gather_numpy(img, 32, 8)
    d = torch.from_numpy(img).cuda()
    assert np.array_equal(tile_gather(d, 32, 8).cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(tile_gather(d, 32, 8, 1, 2).cpu().numpy().view(np.uint32), want[1:3].view(np.uint32))
    for bad in (lambda: tile_gather(d, 40, 8), lambda: tile_gather(d, 32, 17), lambda: tile_gather(d, 32, 8, 3, 2),
                lambda: tile_gather(d.float(), 32, 8), lambda: tile_gather(torch.from_numpy(img), 32, 8)):
        with pytest.raises(_lib.UnetdcError):
            bad()


def blend_abi(tiles, h, w, T, O):
    """unetdc_tile_blend_f32 into a canaried [h, w] buffer that holds NaN everywhere before the launch."""
    from unet_dc_segmentation_amd import _lib
    yo, xo = plan_dev(h, w, T, O)
    assert tiles.shape == (len(yo) * len(xo), T, T) and tiles.dtype == np.float32
    src, out = canaried_like(tiles, align=16), Canaried(h * w * 4, align=4)
    out.view(torch.float32, h, w).fill_(float("nan"))
    _lib.call("unetdc_tile_blend_f32", src.ptr, T, O, yo.data_ptr(), len(yo), xo.data_ptr(), len(xo), out.ptr, h, w, _stream())
    torch.cuda.synchronize()
    out.check("blended map")
    src.check("tile probabilities")
    return out.numpy(np.float32, h, w)


BLEND = [(37, 53, 32, 8), (20, 70, 32, 16), (5, 9, 32, 0), (1, 1, 32, 8), (65, 65, 32, 16), (100, 150, 64, 16), (64, 64, 64, 16)]


@pytest.mark.parametrize("h,w,T,O", BLEND)
def test_blend_exact_round_trip(h, w, T, O):
    """Tiles cut from an image of values k / 256 blend back to it bit for bit (no fp32 operation rounds: test_tiling_cpu.py,
    test_exact_round_trip): any origin, offset or weight error shows.  The folded part of the tiles of a small image is filled
    with NaN: it is never read."""
    plane = image(h, w, 1, seed=h * w)[..., 0].astype(np.float32) / np.float32(256)
    yo, xo = tl.tile_plan(h, w, T, O)
    r = np.arange(T)
    tiles = np.stack([plane[tl.fold(y0 + r, h)][:, tl.fold(x0 + r, w)] for y0 in yo for x0 in xo])
    tiles[:, h:, :] = np.nan
    tiles[:, :, w:] = np.nan
    got = blend_abi(tiles, h, w, T, O)
    assert not np.isnan(got).any()                                                # fully written, nothing read from the padding
    assert np.array_equal(got.view(np.uint32), plane.view(np.uint32))


@pytest.mark.parametrize("h,w,T,O", BLEND)
def test_blend_accuracy_and_determinism(h, w, T, O):
    yo, xo = tl.tile_plan(h, w, T, O)
    tiles = np.random.default_rng(h + w).random((len(yo) * len(xo), T, T)).astype(np.float32)
    a, b = blend_abi(tiles, h, w, T, O), blend_abi(tiles, h, w, T, O)
    assert not np.isnan(a).any() and np.array_equal(a.view(np.uint32), b.view(np.uint32))             # two runs, bit-equal
    err = float(np.abs(a - tl.blend_numpy64(tiles, h, w, T, O)).max())
    print(f"[blend {h}x{w} T{T} O{O}] max |device - fp64| = {err:.3e}")
    assert err < 1e-6
    assert np.array_equal(a.view(np.uint32), tl.blend_numpy(tiles, h, w, T, O).view(np.uint32))       # the same fp32 operations


def test_blend_past_the_grid_cap():
    """2048 x 2048 pixels from 5 x 5 tiles of 512: 16384 workgroups' worth of pixels on a grid capped at 2048, so every thread
    takes eight trips of the grid-stride loop."""
    from unet_dc_segmentation_amd.tiling import tile_blend
    h = w = 2048
    yo, xo = tl.tile_plan(h, w, 512, 64)
    assert len(yo) == len(xo) == 5
    tiles = np.random.default_rng(5).random((25, 512, 512), dtype=np.float32)
    got = tile_blend(torch.from_numpy(tiles).cuda(), h, w, 512, 64).cpu().numpy()
    want = tl.blend_numpy64(tiles, h, w, 512, 64)
    err = float(np.abs(got - want).max())
    print(f"[blend 2048x2048] max |device - fp64| = {err:.3e}")
    assert got.shape == (h, w) and not np.isnan(got).any() and err < 1e-6


def test_abi_refuses_bad_arguments_before_any_launch():
    from unet_dc_segmentation_amd import _lib
    lib = _lib.load()
    yo, xo = plan_dev(37, 53, 32, 8)
    img, tiles = Canaried(37 * 53 * 3, align=16), Canaried(4 * 3 * 32 * 32 * 4, align=16)
    probs, out = Canaried(4 * 32 * 32 * 4, align=16), Canaried(37 * 53 * 4, align=4)

    def gather(**kw):
        a = dict(src=img.ptr, h=37, w=53, c=3, dst=tiles.ptr, T=32, yo=yo.data_ptr(), ny=2, xo=xo.data_ptr(), nx=2, t0=0, count=4)
        a.update(kw)
        return lib.unetdc_tile_gather_u8_to_chw_f32(a["src"], a["h"], a["w"], a["c"], a["dst"], a["T"], a["yo"], a["ny"], a["xo"],
                                                    a["nx"], a["t0"], a["count"], _stream())

    def blend(**kw):
        a = dict(src=probs.ptr, T=32, O=8, yo=yo.data_ptr(), ny=2, xo=xo.data_ptr(), nx=2, dst=out.ptr, h=37, w=53)
        a.update(kw)
        return lib.unetdc_tile_blend_f32(a["src"], a["T"], a["O"], a["yo"], a["ny"], a["xo"], a["nx"], a["dst"], a["h"], a["w"], _stream())

    for kw, word in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(yo=None), "null"), (dict(xo=None), "null"),
                     (dict(h=0), "geometry"), (dict(w=16385), "geometry"), (dict(c=5), "geometry"), (dict(c=0), "geometry"),
                     (dict(T=40), "limits"), (dict(T=0), "limits"), (dict(T=8192), "limits"), (dict(ny=0), "geometry"),
                     (dict(t0=-1), "limits"), (dict(count=0), "limits"), (dict(t0=2, count=3), "limits"),
                     (dict(dst=tiles.ptr + 4), "aligned")):
        assert gather(**kw) == -1 and word.encode() in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    for kw, word in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(yo=None), "null"), (dict(xo=None), "null"),
                     (dict(h=0), "geometry"), (dict(w=16385), "geometry"), (dict(T=40), "limits"), (dict(T=-16), "limits"),
                     (dict(O=-1), "limits"), (dict(O=17), "limits"), (dict(nx=0), "geometry"), (dict(ny=1025), "geometry")):
        assert blend(**kw) == -1 and word.encode() in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    torch.cuda.synchronize()
    assert tiles.untouched() and out.untouched()                                   # a refused call has written nothing
    assert gather() == 0 and blend() == 0
    torch.cuda.synchronize()
    tiles.check("tile buffer")
    out.check("blended map")


# ---- predict_tiled ------------------------------------------------------------------------------------------------------------
def seeded_net():
    from models.model_2 import UNetDC
    from oracle import recipe
    torch.manual_seed(0)
    m = UNetDC(3, 1)
    recipe.perturb_bn(m.state_dict(), 5)
    return m.eval()


def test_predict_tiled_against_its_own_tiles_and_the_cpu_path():
    """80 x 112, T 48, O 16, 4 tiles per forward: 2 x 3 tiles in chunks of 4 + 2 (two engine shapes)."""
    import copy
    from unet_dc_segmentation_amd.tiling import predict_tiled, tile_gather
    h, w, T, O, batch = 80, 112, 48, 16, 4
    img = image(h, w, 3, seed=11)
    cpu_net = seeded_net()
    net = copy.deepcopy(cpu_net).cuda().eval()
    d = torch.from_numpy(img).cuda()
    got = predict_tiled(net, d, T, O, batch)
    assert got.shape == (h, w) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    assert len(net._engines) == 2 and sum(len(v) for v in net._engines.values()) <= net.MAX_ENGINES
    tiles = tile_gather(d, T, O)
    assert tuple(tiles.shape) == (6, 3, T, T)
    with torch.no_grad():                                                          # the HIP module's own outputs, same chunks
        own = torch.cat([net(tiles[0:4])[:, 0].clone(), net(tiles[4:6])[:, 0].clone()]).cpu().numpy()
    e_own = float(np.abs(got - tl.blend_numpy64(own, h, w, T, O)).max())
    ref = tl.predict_tiled_cpu(cpu_net, img, T, O, batch)
    e_cpu = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"[predict_tiled] max |device - fp64 blend of its own tiles| = {e_own:.3e}, max |device - CPU path| = {e_cpu:.3e}")
    assert ref.std() > 1e-3                                                        # the map is not flat
    assert e_own < 1e-6
    assert e_cpu < FP32_PROB_BAR
    again = predict_tiled(net, d, T, O, batch).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


BF16_PROB_BAR_EMU, BF16_PROB_BAR_F32 = 2e-2, 3e-2    # the project's bf16 probability bars (header of tests/test_gpu_e2e.py): against
#                                                      the bf16-storage emulation of the reference and against the fp32 reference.
#                                                      The blend is a convex combination of tile probabilities, so a bar that
#                                                      holds per tile pixel holds for the blended map unchanged.


def test_predict_tiled_bf16_against_both_oracles():
    """The geometry of the fp32 test above (80 x 112, T 48, O 16, chunks of 4 + 2 tiles) with set_compute_dtype("bf16"): what
    quantify_droplets_batch.py --tile 48 --dtype bf16 runs.  The comparison maps are the fp64 blends of the CPU oracle's outputs
    on the gather_numpy tiles, once with bf16 storage emulated and once in plain fp32.  Measured on MI355X: 9.1e-4 against the
    emulation, 6.7e-4 against fp32, 5.3e-8 against the fp64 blend of the device's own tile outputs."""
    import copy
    from oracle import unetdc_torch_cpu as otc
    from unet_dc_segmentation_amd.tiling import predict_tiled, tile_gather
    h, w, T, O, batch = 80, 112, 48, 16, 4
    img = image(h, w, 3, seed=11)
    cpu_net = seeded_net()
    sd = {k: v.detach().clone() for k, v in cpu_net.state_dict().items()}
    net = copy.deepcopy(cpu_net).cuda().eval()
    net.set_compute_dtype("bf16")
    d = torch.from_numpy(img).cuda()
    got = predict_tiled(net, d, T, O, batch)
    assert got.shape == (h, w) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    assert len(net._engines) == 2 and sum(len(v) for v in net._engines.values()) <= net.MAX_ENGINES
    tiles = tile_gather(d, T, O)
    assert tuple(tiles.shape) == (6, 3, T, T)
    with torch.no_grad():                                                          # the HIP module's own bf16 outputs, same chunks
        own = torch.cat([net(tiles[0:4])[:, 0].clone(), net(tiles[4:6])[:, 0].clone()]).cpu().numpy()
    e_own = float(np.abs(got - tl.blend_numpy64(own, h, w, T, O)).max())
    host_tiles = torch.from_numpy(tl.gather_numpy(img, T, O))
    maps = {}
    with torch.no_grad():                                                          # eval mode: a tile's output does not depend on its chunk
        for tag, emu in (("emu", True), ("f32", False)):
            p = otc.unet_forward(host_tiles, sd, dict(cpu_net.DILATIONS), train=False, emulate_bf16=emu)[:, 0].numpy()
            maps[tag] = tl.blend_numpy64(p, h, w, T, O)
    e_emu = float(np.abs(got.astype(np.float64) - maps["emu"]).max())
    e_f32 = float(np.abs(got.astype(np.float64) - maps["f32"]).max())
    print(f"[predict_tiled bf16] max |device - fp64 blend of its own tiles| = {e_own:.3e}, max |device - bf16-storage oracle| = "
          f"{e_emu:.3e}, max |device - fp32 oracle| = {e_f32:.3e}")
    assert maps["f32"].std() > 1e-3                                                # the map is not flat
    assert e_own < 1e-6
    assert e_emu < BF16_PROB_BAR_EMU
    assert e_f32 < BF16_PROB_BAR_F32
    again = predict_tiled(net, d, T, O, batch).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


# ---- script -------------------------------------------------------------------------------------------------------------------
def test_script_tile_on_the_device(tmp_path, monkeypatch):
    """quantify_droplets_batch.main --tile on the device against the same entry point's CPU rule (predict_tiled_cpu): the masks
    agree on every pixel whose CPU probability lies more than the fp32 bar from the threshold, and those are at least 95 % of the
    pixels (the head bias is calibrated so that the threshold cuts through the middle of the map; at this gain the CPU reference
    alone keeps 2.4 % of the pixels inside the band).  A second run adds the split, shape and hole-filling stages."""
    import pandas as pd
    from PIL import Image
    import quantify_droplets_batch as q
    from tests.test_tiling_cpu import SIZES, calibrated_checkpoint, write_images
    from utils.data_loader import rolling_ball_correction_rgb
    assert q.DEVICE == "cuda"
    img_dir = tmp_path / "imgs"
    write_images(img_dir)
    ck, model = calibrated_checkpoint(tmp_path, img_dir, 15, 64, 16, 0.3)
    args = ["--img_dir", str(img_dir), "--ckpt_path", str(ck), "--batch", "4", "--prob_thresh", "0.3", "--skip_excel",
            "--skip_histogram", "--background_radius", "15", "--tile", "64", "--tile_overlap", "16"]
    out = q.main(args + ["--out_dir", str(tmp_path / "gpu")])
    masks = []
    for i, (h, w) in enumerate(SIZES):
        m = np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0
        im = rolling_ball_correction_rgb(np.array(Image.open(img_dir / f"im{i}.png").convert("RGB")), 15)
        p = tl.predict_tiled_cpu(model, im, 64, 16, 4).astype(np.float64)
        guard = np.abs(p - 0.3) > FP32_PROB_BAR
        excluded = 1.0 - float(guard.mean())
        print(f"[script --tile im{i}] excluded {excluded:.4f} of the pixels, mask differs on {int((m != (p > 0.3)).sum())} pixels")
        assert m.shape == (h, w) and 0.1 < m.mean() < 0.9
        assert excluded <= 0.05
        assert np.array_equal(m[guard], (p > 0.3)[guard])
        got = pd.read_csv(out / f"im{i}_droplets.csv")
        want = q.quantify(m.astype(np.uint8), 1, None)                             # the tables follow from the masks
        assert len(got) == len(want) and int(got["area"].sum()) == int(want["area"].sum())
        masks.append(m)
    more = q.main(args + ["--out_dir", str(tmp_path / "more"), "--split_touching", "--droplet_shape", "--fill_holes"])
    assert (more / "mask_clean_per_image.csv").exists()
    for i, (h, w) in enumerate(SIZES):
        m = np.array(Image.open(more / "predicted_masks" / f"im{i}_pred.png")) > 0
        lab = np.array(Image.open(more / "predicted_masks" / f"im{i}_labels.png"))
        assert m.shape == (h, w) and np.array_equal(lab > 0, m)
        assert not (masks[i] & ~m).any() and m.sum() >= masks[i].sum()             # filling holes only adds pixels
        got = pd.read_csv(more / f"im{i}_droplets.csv")
        assert {"perimeter", "eccentricity"} <= set(got.columns) and len(got) == int(lab.max())
