"""CPU: the deep-image window.  utils/intensity_window.py against the plain-loop restatement
tests/intensity_ref.py, the flag parsers, the decoder on files Pillow writes here, and quantify_droplets_batch.py on a
directory of 16-bit files with and without --intensity_window."""
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from tests import intensity_ref as ref
from utils import intensity_window as iw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(37, 53, 1), (37, 53, 3), (5, 7, 4), (1, 300, 2)]


@pytest.mark.parametrize("name", ref.VALUE_SETS)
@pytest.mark.parametrize("shape", SMALL)
def test_ranks_and_window_match_the_restatement(name, shape):
    arr = ref.value_set(name, *shape)
    c = shape[2]
    for ranks, ppm in ref.RANK_LISTS.items():
        want = ref.ranks_of(name, *shape, ranks)
        got = np.stack(iw.ranks_numpy(arr, ppm))
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, shape, ranks)
    value = ref.ranks_of(name, *shape, "five")[0]
    for levels in (value[:, [1, 3]], value[:, [0, 4]], np.tile([[300, 300]], (c, 1)), np.tile([[900, 20]], (c, 1)),
                   np.tile([[0, 65535]], (c, 1)), np.tile([[-5, 70000]], (c, 1))):
        for dc in ([c, 3] if c == 1 else [c]):
            got = iw.window_numpy(arr, levels, dc)
            assert got.dtype == np.uint8 and np.array_equal(got, ref.window_ref(arr, levels, dc)), (name, shape, levels.tolist(), dc)


def test_all_equal_image_gives_zeros_and_the_full_count():
    arr = ref.value_set("equal", 37, 53, 3)
    value, below, equal = iw.ranks_numpy(arr, ref.RANK_LISTS["five"])
    assert (below == 0).all() and (equal == 37 * 53).all() and np.array_equal(value[:, 0], arr[0, 0])
    u8, rec = iw.deep_to_u8_numpy(arr, iw.WindowSpec(1000, 999000))
    assert np.array_equal(rec["levels"][:, 0], rec["levels"][:, 1]) and not u8.any()


def test_small_counts_take_the_nearest_rank():
    """n = 7 with p = 500000: k = ceil(3.5) = 4; n = 1000 with p = 1: k = max(1, ceil(0.001)) = 1, the minimum."""
    a7 = np.array([50, 10, 70, 30, 20, 60, 40], np.uint16).reshape(1, 7, 1)
    assert iw.rank_index(500000, 7) == 4
    v, b, e = iw.ranks_numpy(a7, [500000])
    assert (int(v[0, 0]), int(b[0, 0]), int(e[0, 0])) == (40, 3, 1) == tuple(int(x[0][0]) for x in ref.ranks_ref(a7, [500000]))
    a1000 = np.random.default_rng(5).integers(9, 65536, 1000).astype(np.uint16).reshape(10, 100, 1)
    a1000[3, 3, 0] = 4
    assert iw.rank_index(1, 1000) == 1
    v, b, e = iw.ranks_numpy(a1000, [1])
    assert (int(v[0, 0]), int(b[0, 0]), int(e[0, 0])) == (4, 0, 1) == tuple(int(x[0][0]) for x in ref.ranks_ref(a1000, [1]))


def test_window_rounds_half_up():
    """255 t / d at a tie: lo = 0, hi = 2 maps 1 to 128 (127.5); hi = 510 maps 1 to 1 (0.5).  Round-to-even or truncation fails both."""
    a = np.array([0, 1, 2, 510, 600], np.uint16).reshape(1, 5, 1)
    assert iw.window_numpy(a, [[0, 2]])[0, :, 0].tolist() == [0, 128, 255, 255, 255]
    assert iw.window_numpy(a, [[0, 510]])[0, :, 0].tolist() == [0, 1, 1, 255, 255]
    assert ref.window_value(1, 0, 2) == 128 and ref.window_value(1, 0, 510) == 1


def test_fast_restatement_agrees_with_the_plain_one():
    for name in ref.VALUE_SETS:
        arr = ref.value_set(name, 37, 53, 3)
        for ppm in ref.RANK_LISTS.values():
            assert ref.ranks_ref(arr, ppm) == tuple(ref.ranks_ref_fast(arr, ppm)), name


def test_planes_max():
    planes = np.random.default_rng(2).integers(0, 65536, (5, 9, 11)).astype(np.uint16)
    assert np.array_equal(iw.planes_max_numpy(planes), ref.planes_max_ref(planes))
    with pytest.raises(ValueError):
        iw.planes_max_numpy(planes.astype(np.int32))


def test_parse_window_accepts_and_refuses():
    assert iw.parse_window("0.1,99.9") == (1000, 999000)
    assert iw.parse_window("0,100") == (0, 1000000)
    assert iw.parse_window(" 2.5 , 97.5 ") == (25000, 975000)
    assert iw.parse_window("0.0001,0.0002") == (1, 2)
    assert iw.parse_window("1e-4,5E1") == (1, 500000)
    for bad in ("0.00001,99", "50,50", "60,40", "-1,99", "1,100.0001", "1", "1,2,3", "a,b", "nan,5", "1,inf", ""):
        with pytest.raises(ValueError):
            iw.parse_window(bad)
    assert iw.parse_levels("100,4000") == (100, 4000)
    for bad in ("4000,100", "5,5", "-1,5", "0,65536", "1.5,7", "7"):
        with pytest.raises(ValueError):
            iw.parse_levels(bad)
    assert iw.parse_page("max") == "max" and iw.parse_page("3") == 3
    with pytest.raises(ValueError):
        iw.parse_page("-1")
    assert iw.spec_from_flags(None, None) is None
    assert iw.spec_from_flags("0.1,99.9", None, "max") == iw.WindowSpec(1000, 999000, None, "max")
    assert iw.spec_from_flags(None, "10,500").levels == (10, 500)
    with pytest.raises(ValueError, match="exclude"):
        iw.spec_from_flags("1,99", "10,500")


def _ramp16(h=64, w=64):
    return (np.arange(h * w, dtype=np.uint32) * 65520 // (h * w - 1)).astype(np.uint16).reshape(h, w)


def test_decode_deep_round_trip(tmp_path):
    a = ref.value_set("uniform", 33, 47, 1)[:, :, 0]
    for name in ("a.png", "a.tif"):
        Image.fromarray(a.copy()).save(tmp_path / name)
        assert Image.open(tmp_path / name).mode.startswith("I;16")
        got, mode = iw.decode_deep_info(tmp_path / name)
        assert got.dtype == np.uint16 and got.shape == (33, 47, 1) and np.array_equal(got[:, :, 0], a) and iw.is_deep(mode)
    pages = [ref.value_set("uniform", 33, 47, 1, seed=s)[:, :, 0].copy() for s in (1, 2, 3)]
    ims = [Image.fromarray(p) for p in pages]
    ims[0].save(tmp_path / "stack.tif", save_all=True, append_images=ims[1:])
    assert np.array_equal(iw.decode_deep(tmp_path / "stack.tif", 2)[:, :, 0], pages[2])
    assert np.array_equal(iw.decode_deep(tmp_path / "stack.tif", 0)[:, :, 0], pages[0])
    assert np.array_equal(iw.decode_deep(tmp_path / "stack.tif", "max")[:, :, 0], np.maximum(np.maximum(pages[0], pages[1]), pages[2]))
    with pytest.raises(ValueError):
        iw.decode_deep(tmp_path / "stack.tif", 3)
    # 32-bit integers are clipped; 8-bit modes are widened: grey stays one channel, colour is what convert("RGB") gives
    wide = np.array([[-7, 0, 65535, 70000]], np.int32)
    Image.fromarray(wide).save(tmp_path / "wide.tif")
    assert iw.decode_deep(tmp_path / "wide.tif")[0, :, 0].tolist() == [0, 0, 65535, 65535]
    g = np.arange(48, dtype=np.uint8).reshape(6, 8)
    Image.fromarray(g).save(tmp_path / "g.png")
    assert np.array_equal(iw.decode_deep(tmp_path / "g.png"), g[:, :, None].astype(np.uint16))
    rgb = np.random.default_rng(0).integers(0, 256, (6, 8, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / "c.png")
    assert np.array_equal(iw.decode_deep(tmp_path / "c.png"), rgb.astype(np.uint16))


def test_pillow_clips_deep_images_without_the_window(tmp_path):
    """The defect the stage removes: convert("RGB") on I;16 clips at 255.  If a later Pillow scales instead, the warning's text
    is wrong and this says so."""
    Image.fromarray(_ramp16()).save(tmp_path / "ramp.png")
    rgb = np.array(Image.open(tmp_path / "ramp.png").convert("RGB"))
    assert (rgb == 255).mean() > 0.99


def _blob16(seed, h=96, w=96):
    """A 12-bit micrograph with bright discs, as uint16 [h, w]: every value above 255, as behind a camera's offset."""
    a = ref.micrograph(h, w, seed).astype(np.int64) // 2 + 300
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(6):
        cy, cx, r = rng.integers(8, h - 8), rng.integers(8, w - 8), rng.integers(2, 7)
        a[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 3900
    return a.astype(np.uint16)


@pytest.fixture()
def quantify_cpu(tmp_path, monkeypatch):
    import quantify_droplets_batch as q
    from models.model_2 import UNetDC
    monkeypatch.setattr(q, "DEVICE", "cpu")
    monkeypatch.setattr(q, "IMG_SIZE", 64)
    torch.manual_seed(0)
    ckpt = tmp_path / "best_UNetDC_focal_model.pth"
    torch.save(UNetDC(3, 1).state_dict(), ckpt)
    common = ["--ckpt_path", str(ckpt), "--batch", "2", "--prob_thresh", "0.3", "--skip_excel", "--skip_histogram",
              "--background_radius", "15"]
    return q, common


def test_quantify_windows_a_16_bit_directory(tmp_path, monkeypatch, quantify_cpu):
    """--intensity_window on the CPU path: intensity_per_image.csv holds the restatement's numbers, and what enters the rolling
    ball (and so the network) is the windowed image, not a white rectangle."""
    q, common = quantify_cpu
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    imgs = {"a.png": _blob16(1), "b.tif": _blob16(2)}
    for name, a in imgs.items():
        Image.fromarray(a).save(img_dir / name)
    seen = []
    real = q.rolling_ball_correction_rgb
    monkeypatch.setattr(q, "rolling_ball_correction_rgb", lambda im, r: (seen.append(im.copy()), real(im, r))[1])
    out = q.main(["--img_dir", str(img_dir), "--out_dir", str(tmp_path / "out"), "--intensity_window", "--save_overlays", *common])
    table = pd.read_csv(out / "intensity_per_image.csv", float_precision="round_trip")
    assert list(table["filename"]) == ["a.png", "b.tif"] and all(m.startswith("I;16") for m in table["mode"])
    ppm = [0, 1000, 500000, 999000, 10 ** 6]
    for i, (name, a) in enumerate(imgs.items()):
        arr = a[:, :, None]
        n = a.size
        value, below, equal = (np.asarray(x) for x in ref.ranks_ref_fast(arr, ppm))
        row = table.iloc[i]
        assert [int(row[f"ch0_{k}"]) for k in ("min", "p_lo", "median", "p_hi", "max")] == value[0].tolist()
        assert (int(row["ch0_lo"]), int(row["ch0_hi"])) == (value[0][1], value[0][3]) and int(row["pixels"]) == n
        assert row["ch0_clipped_low_frac"] == below[0][1] / n
        assert row["ch0_clipped_high_frac"] == (n - below[0][3] - equal[0][3]) / n
        assert int(row["ch0_saturated"]) == 0 and int(row["page"]) == 0
        want = ref.window_ref(arr, [[value[0][1], value[0][3]]], 3)
        assert np.array_equal(seen[i], want)
        # not saturated: the discs (a few percent of the pixels) alone reach 255 and the background keeps its gradient, where
        # the clipped decode of the same file is a white rectangle
        assert (seen[i] == 255).mean() < 0.1 and len(np.unique(seen[i])) > 16
        assert (np.array(Image.open(img_dir / name).convert("RGB")) == 255).all()
        assert np.array(Image.open(out / "predicted_masks" / f"{name[:-4]}_pred.png")).shape == a.shape
        ov = np.array(Image.open(out / "overlays" / f"{name[:-4]}_overlay.png"))
        keep = ~((ov[..., 0] == 0) & (ov[..., 1] == 255) & (ov[..., 2] == 0))
        assert np.array_equal(ov[keep], want[keep])                                      # the overlay is painted on the windowed image
    # fixed levels: the same levels for every image, the ranks still reported
    out2 = q.main(["--img_dir", str(img_dir), "--out_dir", str(tmp_path / "out2"), "--intensity_levels", "200,3000", *common])
    t2 = pd.read_csv(out2 / "intensity_per_image.csv")
    assert list(t2["ch0_lo"]) == [200, 200] and list(t2["ch0_hi"]) == [3000, 3000] and list(t2["ch0_max"]) == list(table["ch0_max"])
    assert np.array_equal(seen[-1], ref.window_ref(imgs["b.tif"][:, :, None], [[200, 3000]], 3))
    with pytest.raises(SystemExit):
        q.main(["--img_dir", str(img_dir), "--out_dir", str(tmp_path / "o3"), "--intensity_window", "--intensity_levels", "1,2", *common])
    with pytest.raises(SystemExit):
        q.main(["--img_dir", str(img_dir), "--out_dir", str(tmp_path / "o4"), "--intensity_window", "5,1", *common])
    assert not (tmp_path / "o3").exists() and not (tmp_path / "o4").exists()


def test_quantify_without_the_flag_warns_once_and_changes_nothing(tmp_path, capsys, quantify_cpu):
    """Two 16-bit files without a window flag: one warning line, and every output equals that of the same run on the 8-bit
    files convert("RGB") makes of them -- what the script computed before the stage existed."""
    q, common = quantify_cpu
    deep, flat = tmp_path / "deep", tmp_path / "flat"
    deep.mkdir()
    flat.mkdir()
    for i in (1, 2):
        a = (_blob16(i) // 16).astype(np.uint16)         # 0..255 with discs at 243: clipping keeps a picture to segment
        a[:4, :4] = 4000                                 # ... and a corner that does clip
        Image.fromarray(a).save(deep / f"im{i}.png")
        Image.fromarray(np.array(Image.open(deep / f"im{i}.png").convert("RGB"))).save(flat / f"im{i}.png")
    capsys.readouterr()
    a = q.main(["--img_dir", str(deep), "--out_dir", str(tmp_path / "a"), *common])
    text = capsys.readouterr().out
    assert text.count("clipped at 255") == 1 and "--intensity_window" in text and "im1.png" in text
    b = q.main(["--img_dir", str(flat), "--out_dir", str(tmp_path / "b"), *common])
    assert "clipped at 255" not in capsys.readouterr().out
    assert not (a / "intensity_per_image.csv").exists()
    assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in b.iterdir())
    for name in ("summary_per_image.csv", "im1_droplets.csv", "im2_droplets.csv"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    for i in (1, 2):
        assert np.array_equal(np.array(Image.open(a / "predicted_masks" / f"im{i}_pred.png")),
                              np.array(Image.open(b / "predicted_masks" / f"im{i}_pred.png")))


def test_host_dataset_windows_deep_files(tmp_path):
    """The host-loader path of train_DC_focal.py: SegmentationDataset with a WindowSpec feeds the windowed image to the rolling ball."""
    from utils.data_loader import SegmentationDataset, resize_image, rolling_ball_correction_rgb
    (tmp_path / "i").mkdir()
    (tmp_path / "m").mkdir()
    a = _blob16(3)
    Image.fromarray(a).save(tmp_path / "i" / "a.tif")
    Image.fromarray(((a > 3000) * 255).astype(np.uint8)).save(tmp_path / "m" / "a.tif")
    spec = iw.WindowSpec(*iw.parse_window("1,99"))
    ds = SegmentationDataset(str(tmp_path / "i"), str(tmp_path / "m"), ["a.tif"], ["a.tif"], size=64, radius=15, intensity=spec)
    x = ds[0][0].numpy()
    value = np.asarray(ref.ranks_ref_fast(a[:, :, None], list(spec.ppm))[0])
    u8 = ref.window_ref(a[:, :, None], [[value[0][1], value[0][3]]], 3)
    want = resize_image(rolling_ball_correction_rgb(u8, 15), 64).astype(np.float32) / 255.0
    assert np.array_equal(x, want.transpose(2, 0, 1))
    import train_DC_focal as t
    args = t.build_parser().parse_args(["--intensity_levels", "10,900", "--page", "max"])
    assert t.intensity_spec(args) == iw.WindowSpec(1000, 999000, (10, 900), "max")
    assert t.intensity_spec(t.build_parser().parse_args([])) is None


def test_python_constants_mirror_the_kernel_source():
    """unet_dc_segmentation_amd/window.py restates the launch constants of csrc/window.hip for the tests' second-trip premise."""
    from unet_dc_segmentation_amd import window as wd
    src = open(os.path.join(ROOT, "unet_dc_segmentation_amd", "csrc", "window.hip")).read()
    for name in ("WIN_THREADS", "WIN_HIST_MAX_GROUPS", "WIN_MAX_GROUPS", "WIN_MAX_RANKS", "WIN_MAX_PLANES"):
        m = re.search(r"constexpr int " + name + r" = (\d+);", src)
        assert m and int(m.group(1)) == getattr(wd, name), name
    assert wd.WIN_MAX_RANKS == iw.MAX_RANKS and wd.WIN_MAX_PLANES == iw.MAX_PLANES
    assert wd.HIST_PIXELS_PER_TRIP == wd.WIN_HIST_MAX_GROUPS * wd.WIN_THREADS * 8
    assert "npix / 8" in src and "grid_for(npix / 8, WIN_THREADS, WIN_HIST_MAX_GROUPS)" in src


def test_workspace_query_and_refusals_on_the_host():
    """Host-only: the query refuses what the call refuses, and every refusal comes before the first HIP call (host memory stands in)."""
    import ctypes
    from unet_dc_segmentation_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    assert lib.unetdc_u16_ranks_workspace(1040, 1388, 1, 5) > 0
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (16385, 5, 1, 1), (5, 5, 5, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 5, 1, 9), (32768, 32768, 1, 1)):
        assert lib.unetdc_u16_ranks_workspace(*bad) == 0, bad
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    need = lib.unetdc_u16_ranks_workspace(8, 8, 3, 2)
    ppm = (ctypes.c_int32 * 8)(0, 10 ** 6, 0, 0, 0, 0, 0, 0)
    out = a + 32768
    call = lambda src, ws, nbytes, c=3, nq=2: lib.unetdc_u16_ranks(src, 8, 8, c, ppm, nq, ws, nbytes, out, out + 256, out + 512, None)  # noqa: E731
    assert call(a, a + 4096, need - 1) == -3 and lib.unetdc_last_error().startswith(b"u16_ranks")
    assert call(a + 2, a + 4096, need - 1) == -3                     # the size check comes before the alignment check
    assert call(a + 2, a + 4096, need) == -1 and b"aligned" in lib.unetdc_last_error()
    assert call(a, a + 4096 + 4, need) == -1 and b"aligned" in lib.unetdc_last_error()
    assert call(a, a + 4096, need, c=5) == -1 and call(a, a + 4096, need, nq=0) == -1 and call(a, a + 4096, need, nq=9) == -1
    for p in (-1, 10 ** 6 + 1):
        ppm[1] = p
        assert call(a, a + 4096, need) == -1 and b"parts per million" in lib.unetdc_last_error()
    assert lib.unetdc_window_u16_to_u8(a, 8, 8, 1, a + 1024, a + 2048, 2, None) == -1
    assert lib.unetdc_window_u16_to_u8(a + 2, 8, 8, 1, a + 1024, a + 2048, 3, None) == -1 and b"aligned" in lib.unetdc_last_error()
    assert lib.unetdc_window_u16_to_u8(a, 8, 8, 1, a + 1024, a + 2048 + 8, 3, None) == -1 and b"aligned" in lib.unetdc_last_error()
    assert lib.unetdc_planes_max_u16(a, 0, 8, 8, a + 2048, None) == -1 and lib.unetdc_planes_max_u16(a, 257, 8, 8, a + 2048, None) == -1
    assert lib.unetdc_planes_max_u16(a + 2, 2, 8, 8, a + 2048, None) == -1 and b"aligned" in lib.unetdc_last_error()
