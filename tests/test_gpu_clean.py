"""GPU: the mask-cleaning kernels (csrc/clean.hip) through the C ABI against the host path of the same definition
(utils/droplet_clean.py, itself pinned to tests/clean_ref.py and scipy on the CPU), then through droplets.py and the
script.  Integer work: bit-exact.  Every device output sits between canaries."""
import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from tests.clean_ref import named_cases, noise, weak_for
from tests.test_clean_cpu import ring_probs
from tests.test_split_cpu import FixedProbs, files, noise_mask  # noqa: F401
from utils.droplet_clean import COUNT_NAMES, clean_mask

pytestmark = pytest.mark.gpu

CANARY8 = 0xA5
CANARY32 = -0x35014542            # 0xCAFEBABE as int32
PAD = 24


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_clean(strong, weak, limit, counts=True, in_place=None, ws_bytes=None, ws=None):
    """-> (mask, counts list or None).  out_mask is a plane with two canary rows above and below, out_counts has PAD canary
    words on both sides; in_place = "strong" / "weak" makes that input the output plane;
    ws: a prepared Canaried view (tests/image_canaries.py) to use as the workspace, its guards checked here."""
    from unet_dc_segmentation_amd import _lib
    h, w = strong.shape
    lib = _lib.load()
    nbytes = lib.unetdc_mask_clean_workspace(h, w) if ws_bytes is None else ws_bytes
    if ws is None:
        wbuf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        wptr = wbuf.data_ptr()
    else:
        wptr, nbytes = ws.ptr, ws.nbytes
    buf = torch.full(((h + 4) * w,), CANARY8, dtype=torch.uint8, device="cuda")
    out = buf[2 * w:(h + 2) * w]
    s = torch.from_numpy(np.ascontiguousarray(strong)).cuda()
    k = None if weak is None else torch.from_numpy(np.ascontiguousarray(weak)).cuda()
    if in_place == "strong":
        out.copy_(s.flatten())
        s = out
    elif in_place == "weak":
        out.copy_(k.flatten())
        k = out
    cnt = torch.full((4 + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    _lib.call("unetdc_mask_clean", s.data_ptr(), None if k is None else k.data_ptr(), h, w, limit, wptr, nbytes,
              out.data_ptr(), cnt[PAD:].data_ptr() if counts else None, stream())
    if ws is not None:
        ws.check("workspace")
    b = buf.cpu().numpy()
    assert np.all(b[:2 * w] == CANARY8) and np.all(b[(h + 2) * w:] == CANARY8), "write outside the output plane"
    c = cnt.cpu().numpy()
    assert np.all(c[:PAD] == CANARY32) and np.all(c[PAD + 4:] == CANARY32)
    if not counts:
        assert np.all(c == CANARY32)
    return b[2 * w:(h + 2) * w].reshape(h, w), (c[PAD:PAD + 4].tolist() if counts else None)


def all_masks():
    """name -> (strong, weak): the named cases (a weak mask made up where a case has none) and the noise masks."""
    out = {}
    for k, (strong, weak, _) in named_cases().items():
        out[k] = (strong, weak if weak is not None else weak_for(strong))
    for h, w in ((37, 53), (276, 408), (512, 512)):
        weak = noise_mask(h, w, seed=h)
        out[f"noise{h}x{w}"] = (weak & noise(h, w, h, 0.02), weak)
    return out


MASKS = all_masks()
MODES = [("hysteresis", True, 0), ("holes1", False, 1), ("holes5", False, 5), ("holes_all", False, -1), ("both", True, -1),
         ("both5", True, 5)]
_host = {}


def host(name, use_weak, limit):
    key = (name, use_weak, limit)
    if key not in _host:
        strong, weak = MASKS[name]
        m, c = clean_mask(strong, weak, limit) if use_weak else clean_mask(weak, None, limit)
        _host[key] = (m, c.tolist())
    return _host[key]


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_device_equals_host_path(name, mode):
    _, use_weak, limit = mode
    strong, weak = MASKS[name]
    # holes only runs on the weak mask (it has the holes); the other modes take the pair
    if not use_weak:
        strong = weak
    ref = host(name, use_weak, limit)
    got, c = device_clean(strong, weak if use_weak else None, limit)
    assert got.dtype == np.uint8 and np.array_equal(got, ref[0]) and c == ref[1]


@pytest.mark.parametrize("name", sorted(named_cases()))
def test_named_cases_with_their_own_arguments_and_in_place(name):
    strong, weak, limit = named_cases()[name]
    m, c = clean_mask(strong, weak, limit)
    for where in (None, "strong") + (("weak",) if weak is not None else ()):
        got, gc = device_clean(strong, weak, limit, in_place=where)
        assert np.array_equal(got, m) and gc == c.tolist(), where


@pytest.fixture(scope="module")
def full_size():
    """1040 x 1388 near density 0.5 at the finest grain: the most components and the longest parent chains."""
    weak = noise_mask(1040, 1388, seed=9, sigma=0.7, frac=0.5)
    strong = weak & noise(1040, 1388, 9, 0.01)
    return strong, weak, {lim: clean_mask(strong, weak, lim) for lim in (-1, 6)}


@pytest.mark.parametrize("limit", [-1, 6])
def test_full_size_noise_near_half_density(full_size, limit):
    strong, weak, ref = full_size
    got, c = device_clean(strong, weak, limit)
    m, rc = ref[limit]
    assert np.array_equal(got, m) and c == rc.tolist()
    assert rc[0] > 10000 and rc[1] > 4000 and (limit < 0) == (rc[3] == 0)


def test_two_runs_are_bitwise_equal(full_size):
    strong, weak, _ = full_size
    a, b = device_clean(strong, weak, 6), device_clean(strong, weak, 6)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_without_weak_and_without_holes_the_call_is_a_copy():
    m = MASKS["noise276x408"][1]
    got, c = device_clean(m, None, 0)
    assert np.array_equal(got, m) and c == [0, 0, 0, 0]
    got, c = device_clean(m, None, 0, in_place="strong")
    assert np.array_equal(got, m) and c == [0, 0, 0, 0]


def test_out_counts_may_be_null():
    strong, weak = MASKS["noise37x53"]
    for wk, lim in ((weak, -1), (None, 3), (weak, 0), (None, 0)):
        assert np.array_equal(device_clean(strong, wk, lim, counts=False)[0], clean_mask(strong, wk, lim)[0])


def test_bad_arguments_return_einval_and_launch_nothing():
    from unet_dc_segmentation_amd import _lib
    lib = _lib.load()
    h, w = 37, 53
    strong = torch.ones(h * w, dtype=torch.uint8, device="cuda")
    out = torch.full((h * w,), CANARY8, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), CANARY32, dtype=torch.int32, device="cuda")
    need = lib.unetdc_mask_clean_workspace(h, w)
    ws = torch.full((need,), CANARY8, dtype=torch.uint8, device="cuda")

    def call(hh=h, ww=w, nbytes=need, o=out):
        return lib.unetdc_mask_clean(strong.data_ptr(), None, hh, ww, -1, ws.data_ptr(), nbytes, o.data_ptr(), cnt.data_ptr(), stream())
    for kw, msg in ((dict(nbytes=need - 1), b"workspace"), (dict(hh=0), b"geometry"), (dict(ww=16385), b"geometry"),
                    (dict(hh=-1), b"geometry"), (dict(o=strong[7:]), b"overlap")):
        assert call(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    torch.cuda.synchronize()
    assert bool((out == CANARY8).all()) and bool((cnt == CANARY32).all()) and bool((ws == CANARY8).all()) and bool((strong == 1).all())


# ---- droplets.py ----------------------------------------------------------------------------------------------------------
def probs_of(strong, weak):
    return np.where(strong > 0, 0.9, np.where(weak > 0, 0.4, 0.1)).astype(np.float32)


def test_batch_with_mixed_sizes_equals_single_images_and_waits_once(monkeypatch):
    from unet_dc_segmentation_amd.droplets import mask_and_droplets, mask_and_droplets_batch, resize_mask_like_reference
    sizes = [(300, 401), (512, 512), (97, 33), (1040, 1388)]
    weak = [noise_mask(512, 512, seed=40 + i) for i in range(len(sizes))]
    p = np.stack([probs_of(wk & noise_mask(512, 512, seed=50 + i, sigma=6.0, frac=0.3), wk) for i, wk in enumerate(weak)])
    probs = torch.from_numpy(p).cuda()
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
        out = mask_and_droplets_batch(probs, 0.5, sizes, 1, split_depth=2.0, return_labels=True, thresh_low=0.3, max_hole_area=200)
        # the host waits where it did: the clean counts ride in the copy of the droplet counts
        assert calls == plain_calls == {"cpu": 3, "item": 0}
    counts = [o.clean_counts for o in out]
    assert len(out) == len(sizes) and out[0].labels is not None and plain[0].labels is None
    for i, (oh, ow) in enumerate(sizes):
        one = mask_and_droplets(probs[i], 0.5, (oh, ow), 1, split_depth=2.0, return_labels=True, thresh_low=0.3, max_hole_area=200)
        assert torch.equal(one.mask, out[i].mask) and torch.equal(one.labels, out[i].labels)
        for x, y in zip(list(one)[1:], list(out[i])[1:]):
            assert np.array_equal(x, y)
        assert one.clean_counts.shape == (4,) and np.array_equal(one.clean_counts, counts[i])
        # ... and equal the host path on the two resized masks
        strong = resize_mask_like_reference((p[i] > 0.5).astype(np.uint8), ow, oh)
        wk = resize_mask_like_reference((p[i] > 0.3).astype(np.uint8), ow, oh)
        assert np.array_equal(plain[i].mask.cpu().numpy(), strong)
        m, c = clean_mask(strong, wk, 200)
        assert np.array_equal(out[i].mask.cpu().numpy(), m) and np.array_equal(counts[i], c)
        assert np.array_equal(out[i].labels.cpu().numpy() > 0, m > 0)
    total = np.sum(counts, axis=0)
    assert total[0] > 0 and total[1] > 0 and total[3] > 0           # all three did something somewhere


def test_options_off_launch_nothing_new_and_change_nothing(monkeypatch):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.droplets import mask_and_droplets, mask_and_droplets_batch
    sizes = [(300, 401), (512, 512)]
    p = np.stack([probs_of(noise_mask(512, 512, seed=70 + i) & noise(512, 512, 80 + i, 0.5), noise_mask(512, 512, seed=70 + i))
                  for i in range(2)])
    probs = torch.from_numpy(p).cuda()
    base = mask_and_droplets_batch(probs, 0.5, sizes, 2, shape=True, return_labels=True)
    base_one = mask_and_droplets(probs[0], 0.5, sizes[0], 2)
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    off = mask_and_droplets_batch(probs, 0.5, sizes, 2, shape=True, return_labels=True, thresh_low=None, max_hole_area=0)
    counts = [o.clean_counts for o in off]
    same = mask_and_droplets_batch(probs, 0.5, sizes, 2, shape=True, return_labels=True, thresh_low=0.5)   # equal: a no-op
    off_one = mask_and_droplets(probs[0], 0.5, sizes[0], 2, thresh_low=None, max_hole_area=0)
    assert names and "unetdc_mask_clean" not in names
    assert [c.tolist() for c in counts] == [[0, 0, 0, 0]] * 2
    for got in (off, same):
        for a, b in zip(got, base):
            assert torch.equal(a.mask, b.mask) and torch.equal(a.labels, b.labels)
            assert all(np.array_equal(x, y) for x, y in zip(list(a)[1:], list(b)[1:]))
            assert a.props.keys() == b.props.keys() and all(np.array_equal(a.props[k], b.props[k]) for k in b.props)
    assert torch.equal(off_one.mask, base_one.mask) and all(np.array_equal(x, y) for x, y in zip(list(off_one)[1:], list(base_one)[1:]))
    assert off_one.labels is None and off_one.props is None and base_one.labels is None and base_one.props is None
    names.clear()
    mask_and_droplets_batch(probs, 0.5, sizes, 2, max_hole_area=-1)
    assert names.count("unetdc_mask_clean") == 2
    with pytest.raises(_lib.UnetdcError):
        mask_and_droplets_batch(probs, 0.5, sizes, 2, thresh_low=0.6)


def test_more_droplets_than_the_first_capacity_with_the_options_on():
    from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
    m = np.full((2, 64, 64), 0.1, np.float32)
    m[0, ::2, ::2] = 0.9                                   # 1024 one-pixel droplets, capacity 100 ...
    m[0, 20:23, 20:23] = 0.9                               # ... one of them a 3 x 3 ring around (21, 21)
    m[0, 21, 21] = 0.1
    m[0, 40, 41] = 0.4                                     # a weak bridge between two of them
    m[1, 10:20, 10:20] = 0.9
    m[1, 12:15, 12:15] = 0.1
    out = mask_and_droplets_batch(torch.from_numpy(m).cuda(), 0.5, [(64, 64)] * 2, 1, max_droplets=100, thresh_low=0.3,
                                  max_hole_area=-1)
    counts = [o.clean_counts for o in out]
    ref = [clean_mask(m[i] > 0.5, m[i] > 0.3, -1) for i in range(2)]
    for i in range(2):
        assert np.array_equal(out[i].mask.cpu().numpy(), ref[i][0]) and np.array_equal(counts[i], ref[i][1])
    from scipy import ndimage
    assert len(out[0].area) == ndimage.label(ref[0][0])[1] > 1000 and counts[0].tolist() == [1, 1, 1, 0]
    assert out[1].area.tolist() == [100] and counts[1].tolist() == [0, 1, 9, 0]


# ---- the script ------------------------------------------------------------------------------------------------------------
def test_cli_cleaning_device_equals_cpu_path(tmp_path, monkeypatch):
    """quantify_droplets_batch.py with both flags and --split_touching --droplet_shape writes the same files on the device as
    on the CPU path, given the same probabilities; the ring of image 0 becomes a disc."""
    import quantify_droplets_batch as q
    from tests.test_split_cpu import run_cli
    assert q.DEVICE == "cuda"
    sizes = ((64, 64), (96, 130), (64, 64))
    probs = torch.from_numpy(ring_probs())[:, None]
    args = ["--prob_thresh_low", "0.3", "--fill_holes", "--split_touching", "--droplet_shape", "--px_per_micron", "3.45"]
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    off = run_cli(tmp_path, monkeypatch, "off", args[3:], device="cuda", sizes=sizes, probs=probs)
    fd = files(dev)
    assert fd == files(cpu) and "mask_clean_per_image.csv" in fd and "mask_clean_per_image.csv" not in files(off)
    for f in fd:
        if f.endswith(".png"):
            assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
        elif f.endswith(".csv"):
            if (cpu / f).stat().st_size < 4:                 # the table of an image without droplets: no columns to parse
                assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
                continue
            a, b =(pd.read_csv(d / f, float_precision="round_trip") for d in (dev, cpu))
            assert list(a.columns) == list(b.columns) and len(a) == len(b), f
            for col in a.columns:
                assert a[col].tolist() == b[col].tolist() or np.array_equal(a[col].to_numpy(), b[col].to_numpy(), equal_nan=True), (f, col)
    counts = pd.read_csv(dev / "mask_clean_per_image.csv")
    assert list(counts.columns) == ["filename", *COUNT_NAMES]
    yy, xx = np.mgrid[0:64, 0:64]
    hole = int(((yy - 22) ** 2 + (xx - 20) ** 2 <= 25).sum())
    assert counts[COUNT_NAMES[1]][0] == 1 and counts[COUNT_NAMES[2]][0] == hole
    t_on, t_off = pd.read_csv(dev / "im0_droplets.csv"), pd.read_csv(off / "im0_droplets.csv")
    assert t_on["area"][0] == t_off["area"][0] + hole
    mask = np.array(Image.open(dev / "predicted_masks" / "im0_pred.png"))
    assert mask[22, 20] == 255 and np.array(Image.open(off / "predicted_masks" / "im0_pred.png"))[22, 20] == 0
