"""CPU: scale jitter and foreground-aware windows of native-resolution training (utils/crops.py) -- the
scaled window and gather against a plain-loop restatement (tests/crop_scale_ref.py), the identity at T = S, the orientation of
the resize, the draws of draw_crop_fg, the command-line refusals and the C ABI of unetdc_crop_gather_scaled."""
import ctypes
import os

import numpy as np
import pytest

from tests import crop_scale_ref as sr
from tests import crops_ref as cr
from utils import crops

S = cr.S


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


# ---- the window and the gather --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """{bright: (images, masks, {(img, y0, x0, T): scaled_window_loops})} over every shape, source side and end origin."""
    out = {}
    for bright in (True, False):
        imgs, masks = cr.images(3, bright)
        wins = {(i, y0, x0, T): sr.scaled_window_loops(imgs[i], masks[i], y0, x0, T, S)
                for i, hw in enumerate(cr.SHAPES) for T in sr.TS for y0, x0 in cr.end_origins(*hw, T)}
        out[bright] = (imgs, masks, wins)
    return out


@pytest.mark.parametrize("bright", [True, False])
def test_scaled_window_equals_the_loop_restatement(restated, bright):
    imgs, masks, wins = restated[bright]
    assert len(wins) == 67 and {k[3] for k in wins} == set(sr.TS) and {k[0] for k in wins} == set(range(len(cr.SHAPES)))
    for (i, y0, x0, T), (ew, em) in wins.items():
        win, mwin = crops.window_scaled(imgs[i], masks[i], y0, x0, T, S)
        assert win.dtype == np.float32 and win.shape == (S, S, 3) and mwin.dtype == np.uint8 and mwin.shape == (S, S)
        assert np.array_equal(win.view(np.uint32), (ew.astype(np.float32) / np.float32(255.0)).view(np.uint32)), (i, y0, x0, T)
        assert np.array_equal(mwin, em), (i, y0, x0, T)


@pytest.mark.parametrize("bright", [True, False])
def test_scaled_gather_equals_the_loop_restatement(restated, bright):
    """Every shape, every T, every k and both flips, brightness / contrast on about half."""
    imgs, masks, wins = restated[bright]
    recs = sr.records(seed=3 + bright)
    assert len(recs) == 67 * 16 and {(r["img"], r["y0"], r["x0"], r["T"]) for r in recs} == set(wins)
    assert {(r["params"]["k"], r["params"]["hflip"], r["params"]["vflip"]) for r in recs} == \
        {(k, a, b) for k in range(4) for a in (False, True) for b in (False, True)}
    assert sum(r["params"]["bc"] for r in recs) >= 300
    oi, om = crops.crop_gather_scaled_numpy(imgs, masks, recs, S)
    assert oi.dtype == np.float32 and oi.shape == (len(recs), 3, S, S) and om.shape == (len(recs), 1, S, S)
    for j, r in enumerate(recs):
        ei, em = sr.scaled_sample(*wins[(r["img"], r["y0"], r["x0"], r["T"])], imgs[r["img"]].max(), S, r["params"])
        assert np.array_equal(oi[j].view(np.uint32), ei.view(np.uint32)), r
        assert np.array_equal(om[j], em), r


@pytest.mark.parametrize("elastic", [False, True])
def test_at_t_equal_s_the_scaled_gather_is_the_plain_gather(elastic):
    from tests import augment_ref
    imgs, masks = cr.images(3, bright=True, seed=5)
    recs = cr.records(seed=8)
    fields = None
    if elastic:
        recs = recs[::6]
        fields = [augment_ref.fields(1000 + j, S, S, 3.0, 40.0) for j in range(len(recs))]
        for j, r in enumerate(recs):
            r["params"] = dict(r["params"], elastic=True, field_seed=1000 + j)
    want = crops.crop_gather_numpy(imgs, masks, recs, S, fields)
    got = crops.crop_gather_scaled_numpy(imgs, masks, [dict(r, T=S) for r in recs], S, fields)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


def test_elastic_acts_on_the_scaled_lattice():
    """With a field: scipy's map_coordinates on the S x S window that window_scaled made (reflected at its border)."""
    from scipy import ndimage

    from tests import augment_ref
    imgs, masks = cr.images(3, bright=True, seed=6)
    dx, dy = augment_ref.fields(77, S, S, 3.0, 40.0)
    p = cr.params(hflip=True, k=1, elastic=True, field_seed=77)
    for T in (16, 47):
        oi, om = crops.crop_gather_scaled_numpy(imgs, masks, [dict(img=0, y0=0, x0=3, T=T, params=p)], S, [(dx, dy)])
        win, mwin = crops.window_scaled(imgs[0], masks[0], 0, 3, T, S)
        win, mwin = np.rot90(win[:, ::-1], 1, (0, 1)), np.rot90(mwin[:, ::-1], 1, (0, 1))
        yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        for ch in range(3):
            want = ndimage.map_coordinates(np.ascontiguousarray(win[..., ch]), [yy + dy, xx + dx], order=1, mode="reflect")
            assert np.array_equal(oi[0, ch], want.astype(np.float32))
        assert np.array_equal(om[0, 0], ndimage.map_coordinates(np.ascontiguousarray(mwin), [yy + dy, xx + dx], order=0,
                                                                mode="reflect").astype(np.float32))


def test_the_resize_acts_in_the_windows_own_orientation():
    """T = 16 (first tap -1 at lattice coordinate 0) on an image whose first row and first column differ.  The two axes are not
    interchangeable: the horizontal pass keeps its 19-bit sums, the vertical pass truncates twice ((b * (r >> 4)) >> 16), and
    the border is one tap along x and two clamped taps along y.  So a resize with the axes' rules swapped (the resize of the
    transposed window) or applied after the rotation gives other bytes; the rule resizes first, in the window's orientation.
    (Where both clamped y taps fall on one pixel p the truncated sum is 4 p or 4 p - 1 and (. + 2) >> 2 is p, the one-tap value:
    at the border alone the two rules agree, which is why the whole lattice is compared.)"""
    r = np.random.default_rng(12)
    img = r.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    img[0], img[:, 0] = 250, 3                                # first row bright, first column dark (the corner too)
    mask = (r.random((16, 16)) < 0.4).astype(np.uint8)
    assert sr.axis_taps(0, 16, S, True) == ((0, 1), (2048, 0)) and sr.axis_taps(0, 16, S, False) == ((0, 0), (512, 1536))
    rule = sr.scaled_window_loops(img, mask, 0, 0, 16, S)[0]
    swapped = sr.scaled_window_loops(np.ascontiguousarray(img.transpose(1, 0, 2)), mask.T, 0, 0, 16, S)[0].transpose(1, 0, 2)
    assert (rule != swapped).sum() > 20                       # this image tells the two apart
    assert (rule[0, 4:] >= 249).all() and (rule[4:, 0] == 3).all()
    for k in range(4):
        for hf in (False, True):
            p = cr.params(hflip=hf, k=k)
            oi, _ = crops.crop_gather_scaled_numpy([img], [mask], [dict(img=0, y0=0, x0=0, T=16, params=p)], S)
            base = rule[:, ::-1] if hf else rule
            want = np.rot90(base, k, (0, 1)).astype(np.float32) / np.float32(255.0)
            assert np.array_equal(oi[0], want.transpose(2, 0, 1)), (k, hf)
            # the resize applied AFTER flip and rotation: not the rule
            src = np.rot90(img[:, ::-1] if hf else img, k, (0, 1))
            late = sr.scaled_window_loops(np.ascontiguousarray(src), np.ascontiguousarray(np.rot90(mask, k)), 0, 0, 16, S)[0]
            if k % 2:
                assert not np.array_equal(late.astype(np.float32) / np.float32(255.0), want), (k, hf)


def test_window_scaled_refuses_origins_and_sides_outside_their_ranges():
    imgs, masks = cr.images()
    with pytest.raises(ValueError, match="origin"):
        crops.window_scaled(imgs[0], masks[0], 5, 0, 36, S)            # 40 - 36 = 4
    with pytest.raises(ValueError, match="origin"):
        crops.window_scaled(imgs[0], masks[0], 1, 0, 48, S)            # 40 rows < 48: the origin on that axis is 0
    for T in (15, 65):
        with pytest.raises(ValueError, match="source side"):
            crops.window_scaled(imgs[0], masks[0], 0, 0, T, S)


# ---- t_range and draw_crop_fg ---------------------------------------------------------------------------------------------------
def test_t_range_rounds_once_and_takes_off_float_dust():
    assert crops.t_range(40, (0.55, 1.0)) == (22, 40)
    assert 0.55 * 400 > 220 and 1.13 * 400 < 452                       # the dust: 220.00000000000003, 451.99999999999994
    assert crops.t_range(400, (0.55, 1.13)) == (220, 452)
    assert crops.t_range(32, (0.5, 2.0)) == (16, 64) and crops.t_range(512, (0.5, 2.0)) == (256, 1024)
    assert crops.t_range(32, (1.0, 1.0)) == (32, 32)
    assert crops.t_range(32, (0.51, 1.99)) == (17, 63)                 # ceil(16.32), floor(63.68)
    assert crops.t_range(48, (0.7, 1.3)) == (34, 62)                   # ceil(33.6), floor(62.4)
    for bad in [(0.49, 1), (0.5, 2.01), (1.1, 1.5), (0.6, 0.9), (float("nan"), 1)]:
        with pytest.raises(ValueError):
            crops.t_range(32, bad)


def _fg(mask):
    return np.flatnonzero(mask).astype(np.int32)


def test_draw_crop_fg_is_reproducible_and_independent_of_call_order():
    r = np.random.default_rng(0)
    fg = _fg(r.random((1040, 1388)) < 0.05)
    qs = [(e, q) for e in range(3) for q in range(40)]
    draw = lambda seed, k: crops.draw_crop_fg(seed, k[0], k[1], 1040, 1388, 512, (0.5, 2.0), 0.5, fg)     # noqa: E731
    a = {k: draw(7, k) for k in qs}
    b = {k: draw(7, k) for k in reversed(qs)}
    assert a == b
    assert all(isinstance(v, int) for o in a.values() for v in o)
    assert len(set(a.values())) > 100 and a != {k: draw(8, k) for k in qs}
    # its own stream: the key [seed, epoch, q, 2], the draws in the documented order
    rng = np.random.default_rng([7, 1, 5, 2])
    T = int(rng.integers(256, 1025))
    u = rng.random()
    if u < 0.5:
        py, px = divmod(int(fg[int(rng.integers(0, len(fg)))]), 1388)
        oy, ox = int(rng.integers(0, T)), int(rng.integers(0, T))
        want = (min(max(py - oy, 0), max(1040 - T, 0)), min(max(px - ox, 0), max(1388 - T, 0)), T)
    else:
        want = (int(rng.integers(0, max(1040 - T, 0) + 1)), int(rng.integers(0, max(1388 - T, 0) + 1)), T)
    assert a[(1, 5)] == want
    # draw_crop's stream is untouched: same seed, epoch and sample give unrelated origins
    assert [crops.draw_crop(7, 0, q, 1040, 1388, 512) for q in range(20)] != \
        [crops.draw_crop_fg(7, 0, q, 1040, 1388, 512)[:2] for q in range(20)]


def test_draw_crop_fg_origins_and_sides_stay_in_range_and_reach_both_ends():
    h, w, s = 40, 35, 32
    seen_y, seen_x = set(), set()
    for q in range(3000):                                              # no scale, no foreground: T = S, uniform origins
        y0, x0, T = crops.draw_crop_fg(1, 0, q, h, w, s)
        assert T == s
        seen_y.add(y0)
        seen_x.add(x0)
    assert seen_y == set(range(h - s + 1)) and seen_x == set(range(w - s + 1))
    seen_t = set()
    for q in range(3000):
        y0, x0, T = crops.draw_crop_fg(1, 1, q, h, w, s, (0.6, 1.2))
        seen_t.add(T)
        assert 0 <= y0 <= max(h - T, 0) and 0 <= x0 <= max(w - T, 0)
    assert seen_t == set(range(20, 39))                                # ceil(19.2) .. floor(38.4): both ends, nothing outside
    for hh, ww in [(20, 70), (1, 1), (32, 32), (31, 33)]:
        fg = _fg(np.ones((hh, ww), np.uint8))
        for q in range(100):
            y0, x0, T = crops.draw_crop_fg(1, 2, q, hh, ww, s, (0.5, 2.0), 0.5, fg)
            assert 16 <= T <= 64 and 0 <= y0 <= max(hh - T, 0) and 0 <= x0 <= max(ww - T, 0)
            if hh <= T:
                assert y0 == 0
            if ww <= T:
                assert x0 == 0


@pytest.fixture(scope="module")
def droplet():
    mask = np.zeros((200, 300), np.uint8)
    mask[120:125, 200:205] = 1
    return mask, _fg(mask)


def _holds(mask, y0, x0, T):
    return bool(mask[y0:y0 + T, x0:x0 + T].any())


def test_with_p_fg_1_every_window_contains_a_droplet_pixel_at_many_offsets(droplet):
    mask, fg = droplet
    assert len(fg) == 25 and fg.dtype == np.int32
    offsets = set()
    for q in range(500):
        y0, x0, T, took = crops.draw_crop_fg_branch(3, 0, q, 200, 300, S, (0.5, 2.0), 1.0, fg)
        assert took and 16 <= T <= 64 and 0 <= y0 <= 200 - T and 0 <= x0 <= 300 - T
        assert _holds(mask, y0, x0, T), (q, y0, x0, T)
        assert (y0, x0, T) == crops.draw_crop_fg(3, 0, q, 200, 300, S, (0.5, 2.0), 1.0, fg)
        offsets.add((120 - y0, 200 - x0))
    assert len(offsets) > 400                                          # the droplet is not centred: it lies anywhere in the window


def test_with_p_fg_0_uniform_windows_are_mostly_empty(droplet):
    mask, fg = droplet
    draws = [crops.draw_crop_fg_branch(3, 0, q, 200, 300, S, (0.5, 2.0), 0.0, fg) for q in range(500)]
    assert not any(d[3] for d in draws)
    share = np.mean([_holds(mask, y0, x0, T) for y0, x0, T, _ in draws])
    print(f"share of uniform windows that hold a droplet pixel: {share:.3f}")
    assert share < 0.5


def test_with_p_fg_one_half_the_foreground_branch_is_taken_half_the_time(droplet):
    """2000 samples: 0.5 +- 0.05 is four and a half binomial standard deviations (sqrt(0.25 / 2000) = 0.0112); fixed seeds."""
    mask, fg = droplet
    took = [crops.draw_crop_fg_branch(3, 4, q, 200, 300, S, (0.5, 2.0), 0.5, fg)[3] for q in range(2000)]
    print(f"foreground branch taken: {np.mean(took):.4f}")
    assert abs(np.mean(took) - 0.5) <= 0.05


def test_an_image_without_foreground_always_takes_the_uniform_branch():
    empty = _fg(np.zeros((200, 300), np.uint8))
    assert len(empty) == 0
    for q in range(200):
        y0, x0, T, took = crops.draw_crop_fg_branch(3, 0, q, 200, 300, S, (0.5, 2.0), 1.0, empty)
        assert not took and 0 <= y0 <= 200 - T and 0 <= x0 <= 300 - T
        # ... with the draws of the uniform branch of any other p_fg: u is drawn either way
        assert (y0, x0, T) == crops.draw_crop_fg(3, 0, q, 200, 300, S, (0.5, 2.0), 0.0, None)
    with pytest.raises(ValueError):
        crops.draw_crop_fg(3, 0, 0, 200, 300, S, None, 0.5, None)          # p_fg > 0 needs the indices
    with pytest.raises(ValueError):
        crops.draw_crop_fg(3, 0, 0, 200, 300, S, None, 1.5, empty)


# ---- command line -----------------------------------------------------------------------------------------------------------------
def _argv(tmp_path, *extra):
    missing = str(tmp_path / "no_such_dir")
    return ["--image_dir", missing + "_images", "--mask_dir", missing + "_masks", "--ckpt_path", str(tmp_path / "ck.pth"), *extra]


CROP = ["--crop", "64", "--device_data", "--device", "cuda"]


@pytest.mark.parametrize("extra,word", [
    (["--crop_scale", "0.5", "2", "--device_data", "--device", "cuda"], "--crop_scale needs --crop"),
    (["--crop_fg", "0.5", "--device_data", "--device", "cuda"], "--crop_fg needs --crop"),
    (CROP + ["--crop_scale", "0.4", "1.5"], "--crop_scale"),
    (CROP + ["--crop_scale", "0.5", "2.5"], "--crop_scale"),
    (CROP + ["--crop_scale", "1.2", "1.5"], "--crop_scale"),
    (CROP + ["--crop_scale", "0.6", "0.9"], "--crop_scale"),
    (CROP + ["--crop_scale", "1.5", "0.8"], "--crop_scale"),
    (CROP + ["--crop_scale", "nan", "1.5"], "--crop_scale"),
    (CROP + ["--crop_fg", "-0.1"], "--crop_fg"),
    (CROP + ["--crop_fg", "1.01"], "--crop_fg"),
    (["--crop_scale", "0.4", "1.5"], "--crop_scale"),
    (["--crop_fg", "2"], "--crop_fg"),
])
@pytest.mark.parametrize("entry", ["train_DC_focal", "train"])
def test_scale_and_foreground_refusals_come_before_any_file_is_read(tmp_path, extra, word, entry):
    """The directories do not exist: a refusal that came after a listing would be a FileNotFoundError."""
    import train_DC_focal
    parser = train_DC_focal.build_parser() if entry == "train_DC_focal" else \
        train_DC_focal.build_parser(arch="unet", epochs=50, ckpt="best_UNet_model.pth", loss="bce_dice")     # train.py's
    with pytest.raises(SystemExit) as e:
        train_DC_focal.main(_argv(tmp_path, *extra), parser=parser)
    assert isinstance(e.value.code, str) and word in e.value.code, e.value.code
    assert not os.path.exists(tmp_path / "ck.pth")


def test_scale_and_foreground_flag_defaults():
    import train_DC_focal
    p = train_DC_focal.build_parser()
    a = p.parse_args(["--crop"])
    assert a.crop_scale is None and a.crop_fg == 0.0
    a = p.parse_args(["--crop", "64", "--crop_scale", "0.5", "2", "--crop_fg", "0.25"])
    assert a.crop_scale == [0.5, 2.0] and a.crop_fg == 0.25 and a.crop == 64
    train_DC_focal.check_crop_flags(p.parse_args(CROP + ["--crop_scale", "0.5", "2", "--crop_fg", "1"]))      # the limits pass
    train_DC_focal.check_crop_flags(p.parse_args(CROP + ["--crop_scale", "1", "1", "--crop_fg", "0"]))
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train.py")).read()
    assert "from train_DC_focal import build_parser, main" in src           # train.py shares the parser


def test_train_e2e_passes_both_flags_to_the_crop_arm(monkeypatch):
    import subprocess
    import types

    import importlib.util
    spec = importlib.util.spec_from_file_location("train_e2e", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "train_e2e.py"))
    train_e2e = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_e2e)
    seen = []
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: (seen.append(cmd), types.SimpleNamespace(
        returncode=0, stdout="| 10.0 img/s\n", stderr=""))[1])
    train_e2e.run_arm("crop", 4, "i", "m", 2, 3, "/tmp", 64, ["--crop_scale", "0.5", "2.0", "--crop_fg", "0.5"])
    train_e2e.run_arm("crop", 4, "i", "m", 2, 3, "/tmp", 64)
    train_e2e.run_arm("device_data", 4, "i", "m", 2, 3, "/tmp", 64, ["--crop_fg", "0.5"])
    assert seen[0][seen[0].index("--crop_scale") + 1:][:2] == ["0.5", "2.0"] and seen[0][seen[0].index("--crop_fg") + 1] == "0.5"
    assert "--crop_scale" not in seen[1] and "--crop_fg" not in seen[1] and "--crop_fg" not in seen[2]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_crop_gather_scaled_is_exported_and_its_record_has_the_documented_layout(lib):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.crops import CROP_DTYPE, CROP_SCALED_DTYPE, pack_crops, pack_crops_scaled
    assert hasattr(lib, "unetdc_crop_gather_scaled") and "unetdc_crop_gather_scaled" in _lib.SIGNATURES
    assert _lib.SIGNATURES["unetdc_crop_gather_scaled"] == _lib.SIGNATURES["unetdc_crop_gather"]
    assert lib.unetdc_version() == 2
    assert CROP_SCALED_DTYPE.itemsize == CROP_DTYPE.itemsize == 56
    want = dict(img_off=0, mask_off=8, h=16, w=20, y0=24, x0=28, flags=32, k=36, field=40, alpha=44, beta_max=48, t=52)
    assert {n: CROP_SCALED_DTYPE.fields[n][1] for n in CROP_SCALED_DTYPE.names} == want
    assert CROP_DTYPE.fields["reserved"][1] == 52 and CROP_DTYPE.names[:-1] == CROP_SCALED_DTYPE.names[:-1]
    # pack_crops_scaled: pack_crops' record and seeds, plus t
    ps = [cr.params(k=1, bc=True, alpha=1.1, beta=0.1), cr.params(hflip=True, elastic=True, field_seed=9)]
    args = (ps, [0, 12], [0, 4], [(40, 56), (20, 70)], [(1, 2), (0, 3)], [1.0, 0.5])
    a, sa = pack_crops(*args)
    b, sb = pack_crops_scaled(*args, [47, 16])
    assert np.array_equal(sa, sb) and b["t"].tolist() == [47, 16] and b.dtype == CROP_SCALED_DTYPE
    for n in CROP_DTYPE.names[:-1]:
        assert np.array_equal(a[n], b[n]), n


@pytest.mark.parametrize("name", sorted(sr.REFUSED))
def test_crop_gather_scaled_refuses_on_the_host(lib, name):
    """Validation comes before any HIP call, so it answers without a device (tests/test_crops_cpu.py: where a device is
    visible the buffers are device memory of the full size)."""
    import torch
    sizes = (40 * 56 * 3, 40 * 56, 3 * S * S * 4, S * S * 4)
    if torch.cuda.is_available():
        bufs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in sizes]
        addrs = [b.data_ptr() for b in bufs]
    else:
        bufs = [ctypes.create_string_buffer(n) for n in sizes]
        addrs = [ctypes.addressof(b) for b in bufs]
    ptrs = dict(zip(("images", "masks", "out_img", "out_mask"), addrs))
    assert sr.refused_call(lib, name, ptrs) == -1, name                  # UNETDC_EINVAL
    assert b"crop_gather_scaled" in lib.unetdc_last_error()


def test_an_accepted_empty_call_answers_ok_without_a_device(lib):
    """n = 0 passes validation and launches nothing: the entry point is not refusing everything."""
    bufs = [ctypes.create_string_buffer(64) for _ in range(5)]
    a = [ctypes.addressof(b) for b in bufs]
    assert lib.unetdc_crop_gather_scaled(a[0], 64, a[1], 64, 3, S, a[2], 0, None, 0, a[3], a[4], None) == 0
