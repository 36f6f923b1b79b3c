"""GPU: the droplet split kernels (csrc/split.hip) through the C ABI against scipy's distance transform and the host path of
the same definition (utils/droplet_split.py, itself pinned to tests/split_ref.py on the CPU).  Integer work: bit-exact."""
import math

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

from tests.test_split_cpu import FixedProbs, files, noise_mask, small_masks
from utils import droplet_split as ds

pytestmark = pytest.mark.gpu

CANARY32 = -0x35014542            # 0xCAFEBABE as int32
PAD = 24                          # canary elements before and after each per-droplet output


def stream():
    return torch.cuda.current_stream().cuda_stream


def plane_with_canaries(h, w):
    """[h][w] int32 output view with two canary rows above and below it (one allocation)."""
    buf = torch.full(((h + 4) * w,), CANARY32, dtype=torch.int32, device="cuda")
    return buf, buf[2 * w:(h + 2) * w]


def plane_result(buf, h, w):
    b = buf.cpu().numpy()
    assert np.all(b[:2 * w] == CANARY32) and np.all(b[(h + 2) * w:] == CANARY32), "write outside the output plane"
    return b[2 * w:(h + 2) * w].reshape(h, w)


def workspace(nbytes, ws):
    """-> (owner, address, bytes) of the workspace of a call: a fresh allocation of nbytes, or the Canaried view `ws` a test
    prepared (tests/image_canaries.py; the caller of this checks its guards after the call)."""
    if ws is None:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        return ws, ws.data_ptr(), nbytes
    return ws, ws.ptr, ws.nbytes


def device_edt(mask, ws=None):
    from unet_dc_segmentation_amd import _lib
    h, w = mask.shape
    lib = _lib.load()
    ws, wptr, nbytes = workspace(lib.unetdc_split_workspace(h, w), ws)
    buf, out = plane_with_canaries(h, w)
    m = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    _lib.call("unetdc_edt_sq", m.data_ptr(), h, w, out.data_ptr(), wptr, nbytes, stream())
    if hasattr(ws, "check"):
        ws.check("workspace")
    return plane_result(buf, h, w)


def device_split(mask, h2, min_area=1, max_out=None, labels=True, call="unetdc_split_stats", ws=None):
    """-> (count, rows [(area, sum_row, sum_col, first_index)], label map or None); every output sits between canaries and
    only the first min(count, max_out) entries of the per-droplet outputs may have been written."""
    from unet_dc_segmentation_amd import _lib
    h, w = mask.shape
    lib = _lib.load()
    split = call == "unetdc_split_stats"
    ws, wptr, nbytes = workspace(lib.unetdc_split_workspace(h, w) if split else lib.unetdc_ccl_workspace(h, w), ws)
    cap = h * w if max_out is None else max_out
    m = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    count = torch.full((1 + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    area = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    root = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    sy = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int64, device="cuda")
    sx = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int64, device="cuda")
    lbuf, lab = plane_with_canaries(h, w) if labels and split else (None, None)
    ptrs = [t[PAD:].data_ptr() for t in (count, area, sy, sx, root)]
    if split:
        _lib.call(call, m.data_ptr(), h, w, min_area, h2, wptr, nbytes, *ptrs, None if lab is None else lab.data_ptr(),
                  cap, stream())
    else:
        _lib.call(call, m.data_ptr(), h, w, min_area, wptr, nbytes, *ptrs, cap, stream())
    if hasattr(ws, "check"):
        ws.check("workspace")
    c = count.cpu().numpy()
    assert np.all(c[:PAD] == CANARY32) and np.all(c[PAD + 1:] == CANARY32)
    n = int(c[PAD])
    k = min(n, cap)
    cols = []
    for t in (area, sy, sx, root):
        v = t.cpu().numpy()
        assert np.all(v[:PAD] == CANARY32) and np.all(v[PAD + k:] == CANARY32), "write outside the first min(count, max_out)"
        cols.append(v[PAD:PAD + k].astype(np.int64))
    rows = [tuple(int(x) for x in r) for r in zip(*cols)]
    return n, rows, (None if lbuf is None else plane_result(lbuf, h, w))


def host_rows(mask, h2, min_area=1):
    lab, a, sy, sx, first = ds.split_labels(mask, h2, min_area)
    return lab, [tuple(int(v) for v in r) for r in zip(a, sy, sx, first)]


def masks():
    out = {f"noise{h}x{w}": noise_mask(h, w, seed=h) for h, w in ((37, 53), (276, 408), (512, 512))}
    out.update(small_masks())
    big = noise_mask(1040, 1388, seed=9, sigma=6.0, frac=0.35)
    out["noise1040x1388"] = big
    return out


MASKS = masks()
SMALL = sorted(k for k in MASKS if k != "noise1040x1388")


@pytest.mark.parametrize("name", sorted(MASKS))
def test_edt_equals_scipy(name):
    m = MASKS[name]
    if m.all():
        ref = np.full(m.shape, 2 ** 31 - 1, np.int64)
    else:
        d = ndimage.distance_transform_edt(m)
        ref = np.rint(d * d).astype(np.int64)
    got = device_edt(m)
    assert got.dtype == np.int32 and np.array_equal(got, ref)


def test_edt_without_background_and_with_one_far_background_pixel():
    """No background at 1040 x 1388: UNETDC_EDT_INF everywhere.  One background pixel in a corner: every pixel's scan has to
    reach it (the longest scans the row pass can be asked for)."""
    m = np.ones((1040, 1388), np.uint8)
    assert np.all(device_edt(m) == 2 ** 31 - 1)
    m[1039, 0] = 0
    yy, xx = np.mgrid[0:1040, 0:1388]
    assert np.array_equal(device_edt(m), (yy - 1039) ** 2 + xx ** 2)


def scipy_edt_sq(m):
    if m.all():
        return np.full(m.shape, 2 ** 31 - 1, np.int64)
    d = ndimage.distance_transform_edt(m)
    return np.rint(d * d).astype(np.int64)


def random_mask(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


@pytest.mark.parametrize("w", [63, 64, 65, 255, 256, 257])
def test_edt_at_the_block_seams(w):
    """edt_col_kernel runs 64 columns per block, edt_row_kernel strides a row by 256 threads: one column short of a block,
    a full block, one column into the next."""
    m = random_mask(5, w, 0.7, seed=w)
    assert m[:, w - 1].any() and not m.all()
    assert np.array_equal(device_edt(m), scipy_edt_sq(m))


def test_edt_full_lds_row_and_the_longest_scan():
    """2 x 16384, the promised maximum: the row of g fills 64 KiB of LDS, and with background at (0, 0) only the scan of the
    last pixel runs over the whole row and ends in d^2 = 16383^2 + 1 on the second row."""
    m = np.ones((2, 16384), np.uint8)
    m[0, 0] = 0
    xx = np.arange(16384, dtype=np.int64)
    ref = np.stack([xx * xx, xx * xx + 1])
    assert np.array_equal(scipy_edt_sq(m), ref) and ref[1, -1] == 16383 ** 2 + 1
    assert np.array_equal(device_edt(m), ref)


@pytest.mark.parametrize("shape", [(16384, 1), (1, 16384)], ids=["16384x1", "1x16384"])
def test_edt_one_pixel_wide_at_the_promised_maximum(shape):
    m = random_mask(*shape, 0.7, seed=shape[0])
    assert not m.all()
    assert np.array_equal(device_edt(m), scipy_edt_sq(m))


def test_edt_without_background_at_the_promised_width():
    assert np.all(device_edt(np.ones((3, 16384), np.uint8)) == 2 ** 31 - 1)


@pytest.mark.parametrize("h2", [0, 4])
@pytest.mark.parametrize("shape", [(5, 64), (5, 65), (5, 257), (3, 4097)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_at_the_block_seams(shape, h2):
    """Noise at density 0.6: components that cross the 64-column seams of the distance transform, the 256-thread blocks of the
    per-pixel kernels and the 1024-pixel blocks of the compaction (3 x 4097: one pixel into the thirteenth block)."""
    m = random_mask(*shape, 0.6, seed=shape[1])
    w = shape[1]
    seams = [bool((m[:, x - 1] & m[:, x]).any()) for x in range(64, w, 64)]
    assert not seams or sum(seams) > len(seams) // 2                       # components across most seams (5 x 64 has none inside)
    lab, rows = host_rows(m, h2)
    n, drows, dlab = device_split(m, h2)
    assert n == len(rows) and drows == rows and np.array_equal(dlab, lab)


@pytest.mark.parametrize("h2", [0, 1, 4, 7])
@pytest.mark.parametrize("name", SMALL)
def test_split_equals_host_path(name, h2):
    m = MASKS[name]
    lab, rows = host_rows(m, h2)
    n, drows, dlab = device_split(m, h2)
    assert n == len(rows) and drows == rows
    assert dlab.dtype == np.int32 and np.array_equal(dlab, lab)


@pytest.mark.parametrize("h2,min_area", [(4, 1), (4, 30), (1, 5)])
def test_split_equals_host_path_at_full_size(h2, min_area):
    m = MASKS["noise1040x1388"]
    lab, rows = host_rows(m, h2, min_area)
    n, drows, dlab = device_split(m, h2, min_area)
    assert n == len(rows) and drows == rows and np.array_equal(dlab, lab)
    assert n > ndimage.label(m)[1] or min_area > 1        # the depth does cut something here


@pytest.mark.parametrize("name", SMALL + ["noise1040x1388"])
@pytest.mark.parametrize("min_area", [1, 12])
def test_large_depth_equals_ccl_stats(name, min_area):
    m = MASKS[name]
    h, w = m.shape
    ref = device_split(m, 0, min_area, call="unetdc_ccl_stats")
    for h2 in (2 * math.ceil(math.hypot(h, w)), 2 ** 31 - 1):
        got = device_split(m, h2, min_area, labels=False)
        assert got[0] == ref[0] and got[1] == ref[1], h2


def test_full_mask_is_one_droplet():
    m = np.ones((1040, 1388), np.uint8)
    for h2 in (0, 4):
        n, rows, lab = device_split(m, h2)
        assert n == 1 and rows == [(1040 * 1388, 1388 * sum(range(1040)), 1040 * sum(range(1388)), 0)] and np.all(lab == 1)


def test_count_above_max_out_is_reported_and_only_max_out_written():
    m = MASKS["noise276x408"]
    lab, rows = host_rows(m, 0)
    assert len(rows) > 40
    n, drows, dlab = device_split(m, 0, max_out=17)       # the canary check inside covers entries 17...
    assert n == len(rows) and drows == rows[:17]
    assert np.array_equal(dlab, lab)                       # the label map numbers every droplet all the same
    n0, rows0, _ = device_split(m, 0, max_out=0)
    assert n0 == len(rows) and rows0 == []


def test_two_runs_are_bitwise_equal():
    m = MASKS["noise1040x1388"]
    a, b = device_split(m, 4), device_split(m, 4)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_no_label_map_is_an_option():
    m = MASKS["noise37x53"]
    assert device_split(m, 4, labels=False)[:2] == device_split(m, 4)[:2]


def probs_of(mask):
    return np.where(mask > 0, 0.9, 0.1).astype(np.float32)


def test_batch_with_mixed_sizes_equals_single_images_and_waits_once(monkeypatch):
    from unet_dc_segmentation_amd.droplets import mask_and_droplets, mask_and_droplets_batch
    sizes = [(300, 401), (512, 512), (97, 33), (1040, 1388)]
    base = [noise_mask(512, 512, seed=40 + i) for i in range(len(sizes))]
    probs = torch.from_numpy(np.stack([probs_of(m) for m in base])).cuda()
    calls = {"cpu": 0, "item": 0}
    real_cpu, real_item = torch.Tensor.cpu, torch.Tensor.item

    def cpu(self, *a, **k):
        calls["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)

    def item(self):
        calls["item"] += self.is_cuda
        return real_item(self)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", cpu)
        mp.setattr(torch.Tensor, "item", item)
        plain = mask_and_droplets_batch(probs, 0.5, sizes, 1)
        plain_calls = dict(calls)
        calls.update(cpu=0, item=0)
        out = mask_and_droplets_batch(probs, 0.5, sizes, 1, split_depth=2.0, return_labels=True)
        # the host waits where it did: on the copy of the counts; then the filled part of the areas and of the sums
        assert calls == plain_calls == {"cpu": 3, "item": 0}
    for i, (oh, ow) in enumerate(sizes):
        (mask, a, cy, cx), lab = out[i], out[i].labels
        assert torch.equal(mask, plain[i].mask)
        one = mask_and_droplets(probs[i], 0.5, (oh, ow), 1, split_depth=2.0, return_labels=True)
        assert torch.equal(one.mask, mask) and torch.equal(one.labels, lab)
        for x, y in zip(list(one)[1:], (a, cy, cx)):
            assert np.array_equal(x, y)
        hlab, ha, hsy, hsx, _ = ds.split_labels(mask.cpu().numpy(), 4, 1)
        assert np.array_equal(lab.cpu().numpy(), hlab) and np.array_equal(a, ha)
        assert np.array_equal(cy, hsy / np.maximum(ha, 1)) and np.array_equal(cx, hsx / np.maximum(ha, 1))
        assert len(a) >= len(plain[i].area) and int(a.sum()) == int(plain[i].area.sum())


def test_more_droplets_than_the_first_capacity_with_a_split_depth():
    from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
    m = np.zeros((2, 64, 64), np.float32)
    m[0, ::2, ::2] = 1.0                                   # 1024 one-pixel droplets, capacity 100
    m[1, 10:20, 10:20] = 1.0
    out = mask_and_droplets_batch(torch.from_numpy(m).cuda(), 0.5, [(64, 64)] * 2, 1, max_droplets=100, split_depth=2.0,
                                  return_labels=True)
    assert len(out[0].area) == 1024 and int(out[0].labels.max()) == 1024 and len(out[1].area) == 1


def test_cli_split_touching_device_equals_cpu_path(tmp_path, monkeypatch):
    """quantify_droplets_batch.py --split_touching writes the same tables and label images on the device as on the CPU path,
    given the same 512 x 512 probabilities (the network is replaced by fixed maps on both)."""
    import quantify_droplets_batch as q
    from tests.test_split_cpu import run_cli
    assert q.DEVICE == "cuda"
    sizes = ((512, 512), (300, 401), (1040, 1388), (96, 130), (512, 512))
    p = np.stack([np.where(noise_mask(512, 512, seed=60 + i, sigma=4.0, frac=0.4) > 0, 0.9, 0.1) for i in range(len(sizes))])
    p[4] = 0.1
    probs = torch.from_numpy(p.astype(np.float32))[:, None]
    args = ["--split_touching", "--split_depth", "1.5", "--min_area", "3", "--px_per_micron", "3.45"]
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    fd = files(dev)
    assert fd == files(cpu) and sum(f.endswith("_labels.png") for f in fd) == len(sizes)
    for f in fd:
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    lab = np.array(Image.open(dev / "predicted_masks" / "im2_labels.png"))
    assert lab.shape == (1040, 1388) and lab.max() > 1
