"""GPU: the deep-image window through the C ABI (csrc/window.hip) against the plain-loop restatement
tests/intensity_ref.py, bit for bit.  Outputs and the workspace sit between canaries (tests/image_canaries.py); the workspace
has exactly the queried size and holds 0xFF bytes for the first call of a case and that call's leftovers for the second.

Grid caps: win_hist_kernel takes 8 pixels per thread on at most WIN_HIST_MAX_GROUPS workgroups (HIST_PIXELS_PER_TRIP pixels per
trip: the 1040 x 1388 image is three trips, SECOND_TRIP is built to put its maximum on the second); win_apply_kernel and the
vector form of win_planes_max_kernel take 8 pixels per thread on at most WIN_MAX_GROUPS workgroups, the scalar form one."""
import numpy as np
import pytest
import torch

from tests import intensity_ref as ref
from tests.image_canaries import Canaried, canaried_like, check_all
from unet_dc_segmentation_amd import window as wd
from utils import intensity_window as iw

pytestmark = pytest.mark.gpu

EWORKSPACE = -3
SIDES = [(h, w, c) for h in (63, 64, 65) for w in (127, 128, 129) for c in (1, 3)]
SECOND_TRIP = (65, wd.HIST_PIXELS_PER_TRIP // 64 + 9, 2)
SHAPES = [(1, 1, 1), (1, 300, 3), (300, 1, 2), (3, 5, 4), *SIDES, (257, 301, 3), SECOND_TRIP, (1040, 1388, 1)]
APPLY_PIXELS_PER_TRIP = wd.WIN_MAX_GROUPS * wd.WIN_THREADS * 8


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ppm(ppm):
    return np.asarray(ppm, np.int32)


class Ranks:
    """One image on the device, a workspace of exactly the queried size (0xFF bytes) and canaried outputs for nq requests."""

    def __init__(self, lib, arr, nq):
        self.lib, self.arr, self.nq = lib, arr, nq
        self.h, self.w, self.c = arr.shape
        self.src = canaried_like(arr)
        self.need = lib.unetdc_u16_ranks_workspace(self.h, self.w, self.c, nq)
        assert self.need > 0
        self.ws = Canaried(self.need)
        self.ws.u8.fill_(0xFF)
        self.out = Canaried(3 * self.c * nq * 4)

    def call(self, ppm, src_ptr=None, ws_ptr=None, ws_bytes=None, c=None, nq=None):
        req = _ppm(ppm)
        one = self.c * self.nq * 4
        rc = self.lib.unetdc_u16_ranks(self.src.ptr if src_ptr is None else src_ptr, self.h, self.w, self.c if c is None else c,
                                       req.ctypes.data, len(req) if nq is None else nq, self.ws.ptr if ws_ptr is None else ws_ptr,
                                       self.ws.nbytes if ws_bytes is None else ws_bytes, self.out.ptr, self.out.ptr + one,
                                       self.out.ptr + 2 * one, _stream())
        torch.cuda.synchronize()
        check_all(self.src, self.ws, self.out)
        return rc

    def result(self):
        assert np.array_equal(self.src.numpy(np.uint16, self.h, self.w, self.c), self.arr)       # the image is read only
        return self.out.numpy(np.int32, 3, self.c, self.nq)

    def levels_on_device(self, a, b):
        """int32 [c, 2] device tensor of the values of requests a and b, gathered without a copy to the host."""
        v = self.out.view(torch.int32, 3, self.c, self.nq)[0]
        return torch.stack((v[:, a], v[:, b]), dim=1).contiguous()


def window_call(lib, src, h, w, c, levels_ptr, dc, dst=None, src_ptr=None, dst_ptr=None):
    dst = Canaried(h * w * max(dc, 1)) if dst is None else dst
    rc = lib.unetdc_window_u16_to_u8(src.ptr if src_ptr is None else src_ptr, h, w, c, levels_ptr, dst.ptr if dst_ptr is None else dst_ptr,
                                     dc, _stream())
    torch.cuda.synchronize()
    check_all(src, dst)
    return rc, dst


def _lists_for(shape, k):
    """Every rank list on the small shapes; on the large ones the two five-request lists and one of the others in turn."""
    names = list(ref.RANK_LISTS)
    if shape[0] * shape[1] <= 70000:
        return names
    return ["five", "repeat", ("min", "max", "eight")[k % 3]]


@pytest.mark.parametrize("name", ref.VALUE_SETS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ranks_and_window(lib, shape, name):
    """Ranks for every list, each list twice on one workspace (0xFF bytes, then the first call's leftovers: the second call must
    give the same bytes), then the window with the percentile levels left on the device."""
    h, w, c = shape
    arr = ref.value_set(name, h, w, c)
    n = h * w
    five = None
    for ranks in _lists_for(shape, ref.VALUE_SETS.index(name)):
        ppm = ref.RANK_LISTS[ranks]
        r = Ranks(lib, arr, len(ppm))
        assert r.call(ppm) == 0, lib.unetdc_last_error()
        first = r.result()
        want = ref.ranks_of(name, h, w, c, ranks)
        assert np.array_equal(first, want), (ranks, first.tolist(), want.tolist())
        assert r.call(ppm) == 0, lib.unetdc_last_error()
        assert np.array_equal(r.result(), first), ranks
        if ranks == "five":
            five = r
    value, below, equal = ref.ranks_of(name, h, w, c, "five")
    if name == "equal":
        assert (below == 0).all() and (equal == n).all()
    if name == "ends" and n >= 300:                        # 0 and 65535 present, 65535 repeated: what `saturated` reports
        assert (value[:, 4] == 65535).all() and (equal[:, 4] > 1).all() and (value[:, 0] == 0).all()
    lv = five.levels_on_device(1, 3)
    for dc in ([1, 3] if c == 1 else [c]):
        rc, dst = window_call(lib, five.src, h, w, c, lv.data_ptr(), dc)
        assert rc == 0, lib.unetdc_last_error()
        got = dst.numpy(np.uint8, h, w, dc)
        assert np.array_equal(got, ref.window_ref(arr, value[:, [1, 3]], dc)), dc
        if name == "equal":
            assert not got.any()                         # hi == lo
        assert np.array_equal(got, iw.window_numpy(arr, value[:, [1, 3]], dc))


def test_small_counts(lib):
    """n = 7 with p = 500000 (k = 4) and n = 1000 with p = 1 (k = 1)."""
    a7 = np.array([50, 10, 70, 30, 20, 60, 40], np.uint16).reshape(1, 7, 1)
    r = Ranks(lib, a7, 1)
    assert r.call([500000]) == 0
    assert r.result().ravel().tolist() == [40, 3, 1]
    a = np.random.default_rng(5).integers(9, 65536, 1000).astype(np.uint16).reshape(10, 100, 1)
    a[3, 3, 0] = 4
    r = Ranks(lib, a, 1)
    assert r.call([1]) == 0
    assert r.result().ravel().tolist() == [4, 0, 1]


def test_byte_edges_land_on_each_side(lib):
    """0x00FF / 0x0100 and 0xFEFF / 0xFF00: requests chosen from the value counts so that one lands on the last value below the
    byte edge and the next on the first above it."""
    for name, under, over in (("edge_low", 0x00FF, 0x0100), ("edge_high", 0xFEFF, 0xFF00)):
        arr = ref.value_set(name, 64, 129, 1)
        n = arr.size
        k = int((arr <= under).sum())                    # rank k is `under`, rank k + 1 is `over`
        assert 0 < k < n and (arr == under).any() and (arr == over).any()
        p_under, p_over = k * 10 ** 6 // n, -(-(k + 1) * 10 ** 6 // n)
        assert iw.rank_index(p_under, n) <= k < iw.rank_index(p_over, n)
        r = Ranks(lib, arr, 2)
        assert r.call([p_over, p_under]) == 0
        got = r.result()
        assert got[0, 0].tolist() == [over, under]
        assert np.array_equal(got, np.asarray(ref.ranks_ref_fast(arr, [p_over, p_under]), np.int32))


def test_second_trip_of_the_histogram_passes(lib):
    """The channel maxima lie only behind the first trip's pixels, and the pixel count leaves a tail."""
    h, w, c = SECOND_TRIP
    n, P = h * w, wd.HIST_PIXELS_PER_TRIP
    assert n // 8 > wd.WIN_HIST_MAX_GROUPS * wd.WIN_THREADS and n > P and n % 8 != 0 and max(h, w) <= 16384       # the premise
    arr = ref.value_set("micrograph", h, w, c).copy()
    flat = arr.reshape(n, c)
    flat[P + 5:P + 900] = [60000, 61000]
    flat[n - 1] = [65000, 65001]                         # in the tail
    assert flat[:P].max() < 60000
    ppm = [10 ** 6, 999000, 0, 500000, 999999]
    r = Ranks(lib, arr, 5)
    assert r.call(ppm) == 0
    got = r.result()
    assert got[0, :, 0].tolist() == [65000, 65001] and got[2, :, 0].tolist() == [1, 1]
    assert np.array_equal(got, np.asarray(ref.ranks_ref_fast(arr, ppm), np.int32))


def _levels(rows):
    return canaried_like(np.asarray(rows, np.int32))


def test_window_fixed_levels_ties_and_replication(lib):
    a = np.array([0, 1, 2, 510, 600, 65535, 3, 7, 9], np.uint16).reshape(1, 9, 1)      # nine pixels: a group of eight and the tail
    src = canaried_like(a)
    for levels, want in (([[0, 2]], [0, 128, 255, 255, 255, 255, 255, 255, 255]), ([[0, 510]], [0, 1, 1, 255, 255, 255, 2, 4, 5]),
                         ([[5, 5]], [0] * 9), ([[600, 2]], [0] * 9)):
        lv = _levels(levels)
        for dc in (1, 3):
            rc, dst = window_call(lib, src, 1, 9, 1, lv.ptr, dc)
            assert rc == 0, lib.unetdc_last_error()
            got = dst.numpy(np.uint8, 9, dc)
            assert all(got[:, k].tolist() == want for k in range(dc)), (levels, dc, got.tolist())
            assert want == [ref.window_value(int(v), *levels[0]) for v in a.ravel()]
        lv.check()
    for shape in ((64, 129, 3), (63, 127, 4), (65, 128, 2), (257, 301, 1)):
        arr = ref.value_set("uniform", *shape)
        c = shape[2]
        rows = [[100 * (ch + 1), 60000 - 5000 * ch] for ch in range(c)]
        rows[-1] = [40000, 300] if c > 1 else rows[-1]   # one channel with lo > hi
        lv = _levels(rows)
        src = canaried_like(arr)
        for dc in ([1, 3] if c == 1 else [c]):
            rc, dst = window_call(lib, src, shape[0], shape[1], c, lv.ptr, dc)
            assert rc == 0 and np.array_equal(dst.numpy(np.uint8, shape[0], shape[1], dc), ref.window_ref(arr, rows, dc))


def test_window_second_trip(lib):
    h, w = 129, 16384
    n = h * w
    assert n > APPLY_PIXELS_PER_TRIP and n // 8 > wd.WIN_MAX_GROUPS * wd.WIN_THREADS                               # the premise
    arr = ref.value_set("micrograph", h, w, 1)
    lv = _levels([[200, 3000]])
    rc, dst = window_call(lib, canaried_like(arr), h, w, 1, lv.ptr, 3)
    assert rc == 0
    got = dst.numpy(np.uint8, h, w, 3)
    assert np.array_equal(got, ref.window_ref(arr, [[200, 3000]], 3))
    assert got.reshape(n, 3)[APPLY_PIXELS_PER_TRIP:].any()


def planes_call(lib, planes, P=None, src_ptr=None, dst_ptr=None, dst=None):
    p, h, w = planes.shape
    src = canaried_like(planes)
    dst = Canaried(h * w * 2) if dst is None else dst
    rc = lib.unetdc_planes_max_u16(src.ptr if src_ptr is None else src_ptr(src), p if P is None else P, h, w,
                                   dst.ptr if dst_ptr is None else dst_ptr(dst), _stream())
    torch.cuda.synchronize()
    check_all(src, dst)
    return rc, dst


@pytest.mark.parametrize("shape", [(1, 65, 129), (2, 65, 129), (3, 65, 129), (256, 65, 129), (3, 1, 300), (3, 300, 1), (3, 64, 128),
                                   (2, 513, 517), (2, 129, 16384)], ids=lambda s: "x".join(map(str, s)))
def test_planes_max(lib, shape):
    p, h, w = shape
    if (h, w) == (513, 517):
        assert h * w % 8 and h * w > wd.WIN_MAX_GROUPS * wd.WIN_THREADS          # a second trip of the scalar form
    if (h, w) == (129, 16384):
        assert h * w % 8 == 0 and h * w > APPLY_PIXELS_PER_TRIP                  # ... and of the vector form
    planes = np.random.default_rng(p * h).integers(0, 65536, shape).astype(np.uint16)
    planes[p - 1, h - 1, w - 1] = 65535
    rc, dst = planes_call(lib, planes)
    assert rc == 0, lib.unetdc_last_error()
    got = dst.numpy(np.uint16, h, w)
    assert np.array_equal(got, ref.planes_max_ref(planes)) and np.array_equal(got, iw.planes_max_numpy(planes))


def test_refusals_come_before_any_launch(lib):
    """Bad arguments are UNETDC_EINVAL (-1), a workspace one byte short UNETDC_EWORKSPACE (-3), checked before the alignment; in
    every case the outputs and the workspace keep what they held.  (The bad channel, request, replication and plane counts have
    no workspace to be short of: they are refused as arguments, like every other stage's.)"""
    arr = ref.value_set("uniform", 64, 129, 3)
    r = Ranks(lib, arr, 2)
    ok = [0, 10 ** 6]
    before = r.ws.u8.clone()

    def refused(rc, code):
        assert rc == code, (rc, lib.unetdc_last_error())
        assert r.out.untouched() and torch.equal(r.ws.u8, before)

    refused(r.call(ok, src_ptr=r.src.ptr + 2), -1)
    assert b"aligned" in lib.unetdc_last_error()
    skew = Canaried(r.need, skew=8)
    skew.u8.fill_(0xFF)
    refused(r.call(ok, ws_ptr=skew.ptr, ws_bytes=skew.nbytes), -1)
    assert (skew.u8 == 0xFF).all()
    skew.check()
    refused(r.call(ok, ws_bytes=r.need - 1), EWORKSPACE)
    refused(r.call(ok, src_ptr=r.src.ptr + 2, ws_bytes=r.need - 1), EWORKSPACE)          # the size comes first
    refused(r.call(ok, c=5), -1)
    refused(r.call(ok, nq=0), -1)
    refused(r.call(ok + [5] * 7, nq=9), -1)
    refused(r.call([0, -1]), -1)
    refused(r.call([10 ** 6 + 1, 5]), -1)
    grey = ref.value_set("uniform", 64, 129, 1)
    src, lv = canaried_like(grey), _levels([[0, 65535]] * 4)
    for c, dc, kw in ((1, 2, {}), (5, 5, {}), (0, 1, {}), (1, 1, dict(src_ptr=src.ptr + 2))):
        dst = Canaried(64 * 129 * 5)                       # room for whatever the refused call claims to write
        rc, dst = window_call(lib, src, 64, 129, c, lv.ptr, dc, dst=dst, **kw)
        assert rc == -1 and dst.untouched(), (c, dc, kw, lib.unetdc_last_error())
    rgb = canaried_like(ref.value_set("uniform", 64, 129, 3))
    rc, dst = window_call(lib, rgb, 64, 129, 3, lv.ptr, 1)  # three channels into one
    assert rc == -1 and dst.untouched()
    dst = Canaried(64 * 129 + 16)
    rc, _ = window_call(lib, src, 64, 129, 1, lv.ptr, 1, dst=dst, dst_ptr=dst.ptr + 1)
    assert rc == -1 and dst.untouched() and b"aligned" in lib.unetdc_last_error()
    planes = np.zeros((2, 8, 16), np.uint16)
    for kw in (dict(P=0), dict(P=257), dict(src_ptr=lambda s: s.ptr + 2), dict(dst_ptr=lambda d: d.ptr + 2)):
        rc, dst = planes_call(lib, planes, **kw)
        assert rc == -1 and dst.untouched(), kw


def test_two_runs_give_the_same_bytes(lib):
    arr = ref.value_set("ties", 257, 301, 3)
    outs = []
    for _ in range(2):
        r = Ranks(lib, arr, 5)
        assert r.call(ref.RANK_LISTS["five"]) == 0
        lv = r.levels_on_device(1, 3)
        rc, dst = window_call(lib, r.src, 257, 301, 3, lv.data_ptr(), 3)
        assert rc == 0
        outs.append((r.out.u8.cpu().numpy().tobytes(), dst.u8.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def test_wrappers_and_the_stage_against_numpy():
    """unet_dc_segmentation_amd/window.py: the three calls and deep_to_u8_device, with percentile and with fixed levels."""
    arr = ref.value_set("micrograph", 65, 129, 3)
    t = wd.upload_u16(arr)
    ppm = ref.RANK_LISTS["eight"]
    got = torch.stack(wd.ranks_device(t, ppm)).cpu().numpy()
    assert np.array_equal(got, np.stack(iw.ranks_numpy(arr, ppm)))
    planes = np.random.default_rng(1).integers(0, 65536, (4, 40, 56)).astype(np.uint16)
    assert np.array_equal(wd.planes_max_device(wd.upload_u16(planes)).cpu().numpy().view(np.uint16), iw.planes_max_numpy(planes))
    for spec in (iw.WindowSpec(1000, 999000), iw.WindowSpec(1000, 999000, (300, 2500))):
        for a in (arr, np.ascontiguousarray(arr[:, :, :1])):
            u8, rec = wd.deep_to_u8_device(a, spec)
            want, wrec = iw.deep_to_u8_numpy(a, spec)
            assert u8.shape == want.shape and u8.shape[2] == 3 and np.array_equal(u8.cpu().numpy(), want)
            host = wd.record_host(rec)
            assert np.array_equal(host["ranks"], wrec["ranks"]) and np.array_equal(host["levels"], wrec["levels"])
            assert iw.record_row("a", "I;16", spec, a.shape[0] * a.shape[1], host) == iw.record_row("a", "I;16", spec, a.shape[0] * a.shape[1], wrec)


def test_end_to_end_preprocess_is_bit_identical():
    """A 16-bit 260 x 347 grey image through deep_to_u8_device and preprocess_device_u8, against preprocess_device on
    window_numpy's 8-bit RGB array of the same image: size 64, radius 15, every bit."""
    from unet_dc_segmentation_amd.preprocess import preprocess_device, preprocess_device_u8
    arr = ref.micrograph(260, 347, seed=11)[:, :, None]
    spec = iw.WindowSpec(1000, 999000)
    u8, _ = wd.deep_to_u8_device(arr, spec)
    x, rgb = preprocess_device_u8(u8, 15, 64, return_rgb=True)
    want_u8, _ = iw.deep_to_u8_numpy(arr, spec)
    assert want_u8.shape == (260, 347, 3) and np.array_equal(rgb.cpu().numpy(), want_u8)
    want = preprocess_device(want_u8, 15, 64)
    assert x.shape == (3, 64, 64) and torch.equal(x, want)


def test_device_cache_and_quantify_take_deep_files(tmp_path, monkeypatch):
    """--device_data: both caches window a 16-bit TIFF on the device as the host dataset does on the CPU; quantify_droplets_batch.py
    on the device writes the intensity table of the restatement."""
    import pandas as pd
    from PIL import Image
    from unet_dc_segmentation_amd.device_data import DeviceImageCache, DeviceNativeCache
    from utils.data_loader import SegmentationDataset, rolling_ball_correction_rgb
    (tmp_path / "i").mkdir()
    (tmp_path / "m").mkdir()
    names = ["a.tif", "b.tif"]
    imgs = [ref.micrograph(70, 90, seed=s) + 300 for s in (1, 2)]
    for name, a in zip(names, imgs):
        Image.fromarray(a).save(tmp_path / "i" / name)
        Image.fromarray(((a > 2000) * 255).astype(np.uint8)).save(tmp_path / "m" / name)
    spec = iw.WindowSpec(5000, 995000)
    cache = DeviceImageCache(str(tmp_path / "i"), str(tmp_path / "m"), names, 64, 15, intensity=spec)
    ds = SegmentationDataset(str(tmp_path / "i"), str(tmp_path / "m"), names, names, size=64, radius=15, intensity=spec)
    native = DeviceNativeCache(str(tmp_path / "i"), str(tmp_path / "m"), names, 15, intensity=spec)
    for i, a in enumerate(imgs):
        assert torch.equal(cache.images[i].cpu(), ds[i][0])
        u8 = iw.deep_to_u8_numpy(a[:, :, None], spec)[0]
        assert np.array_equal(native.image(i).cpu().numpy(), rolling_ball_correction_rgb(u8, 15))
    import quantify_droplets_batch as q
    from models.model_2 import UNetDC
    monkeypatch.setattr(q, "IMG_SIZE", 64)
    assert q.DEVICE == "cuda"
    torch.manual_seed(0)
    ckpt = tmp_path / "m.pth"
    torch.save(UNetDC(3, 1).state_dict(), ckpt)
    out = q.main(["--img_dir", str(tmp_path / "i"), "--ckpt_path", str(ckpt), "--out_dir", str(tmp_path / "out"), "--batch", "2",
                  "--skip_excel", "--skip_histogram", "--background_radius", "15", "--intensity_window", "0.5,99.5", "--save_overlays",
                  "--droplet_shape"])
    table = pd.read_csv(out / "intensity_per_image.csv", float_precision="round_trip")
    for i, (name, a) in enumerate(zip(names, imgs)):
        rec = iw.deep_to_u8_numpy(a[:, :, None], spec)[1]
        want = iw.record_row(name, "I;16", spec, a.size, rec)
        got = table.iloc[i].to_dict()
        assert got["mode"].startswith("I;16")
        assert {k: got[k] for k in want if k != "mode"} == {k: v for k, v in want.items() if k != "mode"}
        assert (out / "predicted_masks" / f"{name[:-4]}_pred.png").exists() and (out / "overlays" / f"{name[:-4]}_overlay.png").exists()
