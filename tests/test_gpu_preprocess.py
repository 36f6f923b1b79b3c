"""GPU: input preprocessing kernels (csrc/preprocess.hip) against the numpy restatement of the OpenCV operators in
utils/data_loader.py (the CPU path of the entry points).  Byte arithmetic: the bar is bit-exact."""
import numpy as np
import pytest
import torch

from tests import image_edge_fixtures as fx
from tests.image_canaries import Canaried, canaried_like

pytestmark = pytest.mark.gpu


def _image(rng, h, w, c):
    img = (rng.random((h, w, c)) * 70).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img += (40 * np.sin(yy / 37.0)[..., None] + 40).astype(np.uint8)          # smooth background the opening must follow
    for _ in range(60):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(2, 14)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(180, 255)
    return img


@pytest.mark.parametrize("case", [(96, 130, 3, 15), (257, 301, 3, 50), (64, 64, 1, 1), (200, 90, 3, 2), (150, 150, 4, 127),
                                  (1040, 1388, 3, 50), (7, 5, 3, 3), (40, 33, 2, 9), (130, 70, 1, 128)])
def test_rolling_ball_matches_numpy_restatement(case):
    from unet_dc_segmentation_amd.preprocess import rolling_ball_device
    from utils.data_loader import rolling_ball_correction_rgb
    h, w, c, k = case
    img = _image(np.random.default_rng(h + k), h, w, c)
    ref = rolling_ball_correction_rgb(img, k)
    out = rolling_ball_device(torch.from_numpy(img).cuda(), k).cpu().numpy()
    assert out.dtype == np.uint8 and np.array_equal(out, ref)
    assert k == 1 or (int(ref.max()) == 255 and int(ref.min()) == 0)      # a 1 x 1 element: background = image, all zeros


def test_rolling_ball_flat_image_gives_zeros():
    """max == min after the subtraction: cv2.normalize's scale is 0, the result all zeros."""
    from unet_dc_segmentation_amd.preprocess import rolling_ball_device
    img = np.full((70, 45, 3), 93, np.uint8)
    out = rolling_ball_device(torch.from_numpy(img).cuda(), 9).cpu().numpy()
    assert not out.any()


@pytest.mark.parametrize("shape", [(1040, 1388), (512, 512), (276, 408), (2048, 100), (33, 17)])
def test_resize_to_network_input_matches_numpy_restatement(shape):
    from unet_dc_segmentation_amd.preprocess import resize_to_input_device
    from utils.data_loader import resize_linear_cv2_u8
    h, w = shape
    img = _image(np.random.default_rng(w), h, w, 3)
    ref = resize_linear_cv2_u8(img, 512, 512).astype(np.float32) / 255.0
    out = resize_to_input_device(torch.from_numpy(img).cuda(), 512).cpu().numpy()
    assert out.shape == (3, 512, 512) and out.dtype == np.float32
    assert np.array_equal(out, ref.transpose(2, 0, 1))


# ---- edges, through the C ABI: the output and the workspace sit between canaries, the workspace at exactly the size
# unetdc_rolling_ball_workspace declares, every image pointer 16-byte aligned as the ABI asks --------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rolling_ball_canaried(img, k):
    from unet_dc_segmentation_amd import _lib
    h, w, c = img.shape
    nbytes = _lib.load().unetdc_rolling_ball_workspace(h, w, c)
    src, out, ws = canaried_like(img, align=16), Canaried(h * w * c, align=16), Canaried(nbytes, align=16)
    _lib.call("unetdc_rolling_ball_u8", src.ptr, out.ptr, h, w, c, int(k), ws.ptr, nbytes, _stream())
    torch.cuda.synchronize()
    out.check("rolling-ball output")
    ws.check("rolling-ball workspace")
    src.check("rolling-ball input")
    assert np.array_equal(src.numpy(np.uint8, h, w, c), img)                   # the input is read-only
    return out.numpy(np.uint8, h, w, c)


def _resize_canaried(img, dh, dw):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.preprocess import _resize_tables
    h, w, c = img.shape
    src = torch.from_numpy(img).cuda()
    xo, xa = _resize_tables(w, dw, src.device, True)
    yo, ya = _resize_tables(h, dh, src.device, False)
    out = Canaried(c * dh * dw * 4)
    _lib.call("unetdc_resize_linear_u8_to_chw_f32", src.data_ptr(), h, w, c, out.ptr, dh, dw, xo.data_ptr(), xa.data_ptr(),
              yo.data_ptr(), ya.data_ptr(), _stream())
    torch.cuda.synchronize()
    out.check("resize output")
    return out.numpy(np.float32, c, dh, dw)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("k", [3, 5, 50])
def test_rolling_ball_rounds_ties_to_even(k, channels):
    """Isolated pixels of value 1 .. 10 on black: scale 25.5, so 3 and 7 land on 76.5 and 178.5 -- cv2.normalize rounds half
    to even (76, 178); a kernel that rounds half up gives 77 and 179."""
    from utils.data_loader import rolling_ball_correction_rgb
    img = fx.tie_image(channels)
    want = rolling_ball_correction_rgb(img, k)
    out = _rolling_ball_canaried(img, k)
    assert np.array_equal(out, want)
    for c in range(channels):
        pos = fx.tie_positions(img, c)
        assert [int(out[pos[v] + (c,)]) for v in range(1, 11)] == fx.TIE_EXPECTED


RB_SIDES = [63, 64, 65, 128, 129]          # 64 m and 64 m +- 1: the tile width of morph_kernel
RB_ELEMENTS = [2, 3, 50, 127, 128]


@pytest.mark.parametrize("w", RB_SIDES)
@pytest.mark.parametrize("h", RB_SIDES)
def test_rolling_ball_tile_boundaries(h, w):
    """Every element size and 1 - 4 channels at sides on and around the 64-pixel tile."""
    from utils.data_loader import rolling_ball_correction_rgb
    for c in (1, 2, 3, 4):
        img = _image(np.random.default_rng(1000 * h + 10 * w + c), h, w, c)
        for k in RB_ELEMENTS:
            assert np.array_equal(_rolling_ball_canaried(img, k), rolling_ball_correction_rgb(img, k)), (h, w, c, k)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (1, 300), (300, 1)])
def test_rolling_ball_tiny_and_one_pixel_wide(h, w, c):
    """Fewer than 16 pixels (only the tail branch of subtract_minmax_kernel runs) and one-pixel-wide / -high images."""
    from utils.data_loader import rolling_ball_correction_rgb
    rng = np.random.default_rng(h * 7 + w + c)
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    for k in RB_ELEMENTS:
        assert np.array_equal(_rolling_ball_canaried(img, k), rolling_ball_correction_rgb(img, k)), (h, w, c, k)


@pytest.mark.parametrize("which", ["src", "dst", "workspace"])
def test_rolling_ball_misaligned_pointer_is_an_error_before_any_launch(which):
    from unet_dc_segmentation_amd import _lib
    h, w, c = 20, 31, 3
    img = _image(np.random.default_rng(4), h, w, c)
    nbytes = _lib.load().unetdc_rolling_ball_workspace(h, w, c)
    skew = {which: 4}
    src = canaried_like(img, align=16, skew=skew.get("src", 0))
    out = Canaried(h * w * c, align=16, skew=skew.get("dst", 0))
    ws = Canaried(nbytes, align=16, skew=skew.get("workspace", 0))
    rc = _lib.load().unetdc_rolling_ball_u8(src.ptr, out.ptr, h, w, c, 9, ws.ptr, nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == -1                                                            # UNETDC_EINVAL
    assert b"16-byte aligned" in _lib.load().unetdc_last_error()
    assert out.untouched() and ws.untouched()
    out.check()
    ws.check()


def test_rolling_ball_workspace_too_small_is_an_error_before_any_launch():
    from unet_dc_segmentation_amd import _lib
    h, w, c = 20, 31, 3
    img = _image(np.random.default_rng(4), h, w, c)
    nbytes = _lib.load().unetdc_rolling_ball_workspace(h, w, c)
    src, out, ws = canaried_like(img, align=16), Canaried(h * w * c, align=16), Canaried(nbytes, align=16)
    rc = _lib.load().unetdc_rolling_ball_u8(src.ptr, out.ptr, h, w, c, 9, ws.ptr, nbytes - 1, _stream())
    torch.cuda.synchronize()
    assert rc == -3                                                            # UNETDC_EWORKSPACE
    assert out.untouched() and ws.untouched()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("src_hw,dst_hw", [((276, 408), (384, 384)), ((300, 517), (1024, 1024)), ((130, 97), (64, 64)),
                                           ((97, 61), (80, 200)), ((200, 150), (33, 301)), ((1, 77), (64, 64)),
                                           ((77, 1), (64, 64)), ((1, 1), (5, 7)), ((40, 50), (384, 384)),
                                           ((1, 300), (1, 1024)), ((300, 1), (384, 1))])
def test_resize_any_destination_and_channel_count(src_hw, dst_hw, c):
    """The other network sizes (384, 1024), a small and two non-square destinations, one-row / one-column sources and
    upscales on both axes, 1 - 4 channels: bit-exact against resize_linear_cv2_u8 / 255 in float32."""
    from utils.data_loader import resize_linear_cv2_u8
    (h, w), (dh, dw) = src_hw, dst_hw
    img = np.random.default_rng(h * w + c).integers(0, 256, (h, w, c), dtype=np.uint8)
    ref = resize_linear_cv2_u8(img, dw, dh).astype(np.float32) / np.float32(255.0)
    out = _resize_canaried(img, dh, dw)
    assert ref.dtype == np.float32 and np.array_equal(out.view(np.uint32), ref.transpose(2, 0, 1).view(np.uint32))
