"""CPU: the crop rule of native-resolution training (utils/crops.py) -- the numpy gather against a
plain-loop restatement (tests/crops_ref.py) and against TrainAugment's restatement applied to the sliced window
(tests/augment_ref.py), the crop and evaluation plans, the command-line refusals and the C ABI of unetdc_crop_gather."""
import ctypes
import os

import numpy as np
import pytest

from tests import augment_ref
from tests import crops_ref as cr
from utils import crops
from utils.tiling import tile_plan

S = cr.S


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


# ---- the gather -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bright", [True, False])
def test_gather_equals_the_loop_restatement(bright):
    imgs, masks = cr.images(3, bright)
    recs = cr.records(seed=3 + bright)
    assert {(r["img"], r["y0"], r["x0"]) for r in recs} == {(i, *o) for i, hw in enumerate(cr.SHAPES) for o in cr.end_origins(*hw)}
    assert {(r["params"]["k"], r["params"]["hflip"], r["params"]["vflip"]) for r in recs} == \
        {(k, a, b) for k in range(4) for a in (False, True) for b in (False, True)}
    assert sum(r["params"]["bc"] for r in recs) >= 40
    oi, om = crops.crop_gather_numpy(imgs, masks, recs, S)
    assert oi.dtype == np.float32 and oi.shape == (len(recs), 3, S, S) and om.shape == (len(recs), 1, S, S)
    for j, r in enumerate(recs):
        ei, em = cr.crop_sample_loops(imgs[r["img"]], masks[r["img"]], r["y0"], r["x0"], S, r["params"])
        assert np.array_equal(oi[j].view(np.uint32), ei.view(np.uint32)), r
        assert np.array_equal(om[j], em), r


def test_brightness_uses_the_maximum_of_the_whole_image():
    """The stated deviation: beta_max = beta * (image maximum), also where the window's own maximum is smaller."""
    imgs, masks = cr.images(3, bright=False)
    img = imgs[0]                                                  # 40 x 56, its maximum 231 at (39, 0)
    p = cr.params(bc=True, alpha=1.1, beta=0.15)
    oi, _ = crops.crop_gather_numpy(imgs, masks, [dict(img=0, y0=0, x0=24, params=p)], S)
    win = img[:S, 24:24 + S]
    assert win.max() < img.max() == 231
    want = np.clip(np.float32(1.1) * (win.astype(np.float32) / np.float32(255)) + np.float32(0.15 * crops.image_max(img)), 0, 1)
    assert np.array_equal(oi[0], want.transpose(2, 0, 1).astype(np.float32))
    other = np.clip(np.float32(1.1) * (win.astype(np.float32) / np.float32(255)) + np.float32(0.15 * crops.image_max(win)), 0, 1)
    assert not np.array_equal(oi[0], other.transpose(2, 0, 1).astype(np.float32))


def _sliced_window(img, mask, y0, x0):
    """The window by slicing, an image smaller than the crop extended by np.pad's "reflect": nothing of utils.crops."""
    h, w = mask.shape
    py, px = max(S - h, 0), max(S - w, 0)
    img, mask = np.pad(img, ((0, py), (0, px), (0, 0)), mode="reflect"), np.pad(mask, ((0, py), (0, px)), mode="reflect")
    return img[y0:y0 + S, x0:x0 + S].astype(np.float32) / np.float32(255.0), mask[y0:y0 + S, x0:x0 + S]


@pytest.mark.parametrize("elastic", [False, True])
def test_gather_is_the_augmentation_of_the_sliced_window(elastic):
    """crop_gather_numpy == augment_ref.augment_with_params(window / 255, mask window, params, dx, dy): the crop path is the
    resized path's augmentation at another scale.  The images carry their maximum in every end window (crops_ref.images)."""
    imgs, masks = cr.images(3, bright=True, seed=5)
    recs = cr.records(seed=8)[::3]
    fields = None
    if elastic:
        fields = []
        for j, r in enumerate(recs):
            r["params"] = dict(r["params"], elastic=True, field_seed=1000 + j)
            fields.append(augment_ref.fields(1000 + j, S, S, 3.0, 40.0))
        assert max(np.abs(f[0]).max() for f in fields) > 1.0
    oi, om = crops.crop_gather_numpy(imgs, masks, recs, S, fields)
    for j, r in enumerate(recs):
        win, mwin = _sliced_window(imgs[r["img"]], masks[r["img"]], r["y0"], r["x0"])
        assert win.max() == np.float32(1.0)
        dx, dy = fields[j] if elastic else (None, None)
        ei, em = augment_ref.augment_with_params(win, mwin, r["params"], dx, dy)
        assert np.array_equal(oi[j].view(np.uint32), ei.transpose(2, 0, 1).view(np.uint32)), r
        assert np.array_equal(om[j, 0], em.astype(np.float32)), r


def test_window_refuses_an_origin_outside_its_range():
    imgs, masks = cr.images()
    for y0, x0 in [(-1, 0), (9, 0), (0, 25), (0, -1)]:
        with pytest.raises(ValueError, match="origin"):
            crops.window(imgs[0], masks[0], y0, x0, S)
    with pytest.raises(ValueError, match="origin"):
        crops.window(imgs[2], masks[2], 1, 0, S)                   # 20 rows < S: the origin on that axis is 0


# ---- draw_crop ------------------------------------------------------------------------------------------------------------------
def test_draw_crop_is_reproducible_and_independent_of_call_order():
    qs = [(e, q) for e in range(3) for q in range(40)]
    a = {k: crops.draw_crop(7, k[0], k[1], 1040, 1388, 512) for k in qs}
    b = {k: crops.draw_crop(7, k[0], k[1], 1040, 1388, 512) for k in reversed(qs)}
    assert a == b
    assert all(isinstance(v, int) for o in a.values() for v in o)
    assert len(set(a.values())) > 100                                          # epochs and samples differ
    assert a != {k: crops.draw_crop(8, k[0], k[1], 1040, 1388, 512) for k in qs}


def test_draw_crop_stays_in_range_and_reaches_both_ends():
    h, w, s = 40, 35, 32
    seen_y, seen_x = set(), set()
    for q in range(3000):
        y0, x0 = crops.draw_crop(1, 0, q, h, w, s)
        seen_y.add(y0)
        seen_x.add(x0)
    assert seen_y == set(range(h - s + 1)) and seen_x == set(range(w - s + 1))     # 0 and dim - S included
    for hh, ww in [(20, 70), (1, 1), (32, 32), (31, 33)]:
        for q in range(50):
            y0, x0 = crops.draw_crop(1, 2, q, hh, ww, s)
            assert 0 <= y0 <= max(hh - s, 0) and 0 <= x0 <= max(ww - s, 0)
            if hh <= s:
                assert y0 == 0
            if ww <= s:
                assert x0 == 0


def test_draw_crop_differs_between_reps_and_from_the_augmentation_stream():
    R = 4
    o = [crops.draw_crop(3, 1, crops.sample_number(17, rep, R), 1040, 1388, 512) for rep in range(R)]
    assert len(set(o)) == R
    assert [crops.sample_number(5, rep, 3) for rep in range(3)] == [15, 16, 17]
    with pytest.raises(ValueError):
        crops.sample_number(5, 3, 3)
    # the four-element key: not the first draws of augment.draw_params' generator
    r3, r4 = np.random.default_rng([3, 1, 68]), np.random.default_rng([3, 1, 68, 1])
    assert int(r3.integers(0, 529)) != int(r4.integers(0, 529)) or int(r3.integers(0, 877)) != int(r4.integers(0, 877))
    r4 = np.random.default_rng([3, 1, 68, 1])
    assert crops.draw_crop(3, 1, 68, 1040, 1388, 512) == (int(r4.integers(0, 529)), int(r4.integers(0, 877)))


# ---- eval_plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,s", [(1040, 1388, 512), (48, 80, 32), (30, 44, 32), (32, 32, 32), (1, 1, 32), (33, 65, 32)])
def test_eval_plan_is_the_tile_plan_without_overlap_and_covers_every_pixel(h, w, s):
    plan = crops.eval_plan(h, w, s)
    yo, xo = tile_plan(h, w, s, 0)
    assert plan == [(y0, x0) for y0 in yo for x0 in xo]
    cover = np.zeros((h, w), np.int32)
    for y0, x0 in plan:
        assert 0 <= y0 <= max(h - s, 0) and 0 <= x0 <= max(w - s, 0)
        cover[y0:y0 + s, x0:x0 + s] += 1
    assert cover.min() >= 1


# ---- command line -----------------------------------------------------------------------------------------------------------------
def _argv(tmp_path, *extra):
    missing = str(tmp_path / "no_such_dir")
    return ["--image_dir", missing + "_images", "--mask_dir", missing + "_masks", "--ckpt_path", str(tmp_path / "ck.pth"), *extra]


@pytest.mark.parametrize("extra,word", [
    (["--crop", "64"], "--device_data"),
    (["--crop", "64", "--device_data", "--synthetic", "--device", "cuda"], "--synthetic"),
    (["--crop", "64", "--device_data", "--device", "cpu"], "cannot run on --device cpu"),
    (["--crop", "64", "--device_data", "--device", "cuda", "--in_channels", "1"], "--in_channels 1"),
    (["--crop", "40", "--device_data", "--device", "cuda"], "--crop"),
    (["--crop", "16", "--device_data", "--device", "cuda"], "--crop"),
    (["--crop", "1040", "--device_data", "--device", "cuda"], "--crop"),
    (["--crop", "64", "--crops_per_image", "0", "--device_data", "--device", "cuda"], "--crops_per_image"),
    (["--crops_per_image", "2", "--device_data", "--device", "cuda"], "--crop"),
])
@pytest.mark.parametrize("entry", ["train_DC_focal", "train"])
def test_crop_refusals_come_before_any_file_is_read(tmp_path, extra, word, entry):
    """The directories do not exist: a refusal that came after a listing would be a FileNotFoundError."""
    import train_DC_focal
    parser = train_DC_focal.build_parser() if entry == "train_DC_focal" else \
        train_DC_focal.build_parser(arch="unet", epochs=50, ckpt="best_UNet_model.pth", loss="bce_dice")     # train.py's
    with pytest.raises(SystemExit) as e:
        train_DC_focal.main(_argv(tmp_path, *extra), parser=parser)
    assert isinstance(e.value.code, str) and word in e.value.code, e.value.code
    assert not os.path.exists(tmp_path / "ck.pth")


def test_crop_flag_defaults():
    import train_DC_focal
    p = train_DC_focal.build_parser()
    a = p.parse_args(["--crop"])
    assert a.crop == 512 and a.crops_per_image == 1
    assert p.parse_args(["--crop", "256", "--crops_per_image", "3"]).crop == 256
    assert p.parse_args([]).crop is None
    assert p.parse_args(["--crop", "--device_data"]).crop == 512              # the next flag is not taken for S


def test_train_py_shares_the_flags():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train.py")).read()
    assert "from train_DC_focal import build_parser, main" in src


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_crop_gather_is_exported_and_its_record_has_the_documented_layout(lib):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.crops import CROP_DTYPE
    assert hasattr(lib, "unetdc_crop_gather") and "unetdc_crop_gather" in _lib.SIGNATURES
    assert CROP_DTYPE.itemsize == 56 and CROP_DTYPE.itemsize % 8 == 0
    want = dict(img_off=0, mask_off=8, h=16, w=20, y0=24, x0=28, flags=32, k=36, field=40, alpha=44, beta_max=48)
    assert {n: CROP_DTYPE.fields[n][1] for n in want} == want


@pytest.mark.parametrize("name", sorted(cr.REFUSED))
def test_crop_gather_refuses_on_the_host(lib, name):
    """Validation comes before any HIP call, so it answers without a device: the pointers are host buffers nothing reads.
    Where a device is visible the buffers are device memory of the full size (40 x 56 x 3 image, its mask, 32 x 32 outputs),
    so that a case that slipped through validation would launch on memory it may touch."""
    import torch
    sizes = (40 * 56 * 3, 40 * 56, 3 * cr.S * cr.S * 4, cr.S * cr.S * 4)
    if torch.cuda.is_available():
        bufs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in sizes]
        addrs = [b.data_ptr() for b in bufs]
    else:
        bufs = [ctypes.create_string_buffer(n) for n in sizes]
        addrs = [ctypes.addressof(b) for b in bufs]
    ptrs = dict(zip(("images", "masks", "out_img", "out_mask"), addrs))
    assert cr.refused_call(lib, name, ptrs) == -1, name                  # UNETDC_EINVAL
    assert b"crop_gather" in lib.unetdc_last_error()
