"""GPU: per-droplet confidence and TTA disagreement (csrc/confidence.hip, the envelope kernel of csrc/tta.hip, DESIGN.md section
23) through the C ABI against the host path of the same definition (utils/droplet_confidence.py, utils/tta.py, themselves pinned
to tests/confidence_ref.py on the CPU); then droplets.py and the CLI flag.  Integer work: bit-exact.  Every output sits between
canaries."""
import ctypes

import numpy as np
import pytest
import torch

from tests.image_canaries import Canaried, canaried_like
from tests.test_confidence_cpu import BAND, GEOMETRIES, MAX_OUT, THRESH, fixture, label_map, planes, run_script
from utils import droplet_confidence as dc
from utils import tta

pytestmark = pytest.mark.gpu

NC, NI = len(dc.CONF_QUANTITIES), len(dc.IMAGE_QUANTITIES)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table():
    from unet_dc_segmentation_amd.droplets import _entropy_table
    return _entropy_table(torch.device("cuda", torch.cuda.current_device()))


def device_confidence(lab, p, thresh, band, lo=None, hi=None, max_out=MAX_OUT, maps=False, prefill=None, null_out=False):
    """unetdc_label_confidence -> (rows int64 [NC, max_out], image int64 [NI], entropy map or None, spread map or None).
    prefill: what the rows and the image totals hold before the call (a byte value or an int64 array); the canary pattern
    otherwise."""
    from unet_dc_segmentation_amd import _lib
    h, w = lab.shape
    ph, pw = p.shape
    ins = [canaried_like(np.array(a)) for a in (lab.astype(np.int32), p)]          # copies: the fixtures are read-only
    env = [canaried_like(np.array(a)) for a in (lo, hi)] if lo is not None else []
    out, img = Canaried(NC * max_out * 8, align=8), Canaried(NI * 8, align=8)
    emap = Canaried(h * w, align=1) if maps else None
    smap = Canaried(h * w, align=1) if maps and lo is not None else None
    if isinstance(prefill, int):
        out.u8.fill_(prefill)
        img.u8.fill_(prefill)
    elif prefill is not None:
        out.u8.copy_(torch.from_numpy(prefill[0].reshape(-1).view(np.uint8)))
        img.u8.copy_(torch.from_numpy(prefill[1].reshape(-1).view(np.uint8)))
    _lib.call("unetdc_label_confidence", ins[0].ptr, max_out, h, w, ins[1].ptr, *([e.ptr for e in env] or [None, None]), ph, pw,
              float(thresh), float(band), _table().data_ptr(), None if null_out else out.ptr, img.ptr,
              None if emap is None else emap.ptr, None if smap is None else smap.ptr, _stream())
    torch.cuda.synchronize()
    for v in [*ins, *env, out, img, emap, smap]:
        if v is not None:
            v.check()
    assert np.array_equal(ins[0].numpy(np.int32, h, w), lab) and ins[1].numpy(np.uint32, ph, pw).tobytes() == p.tobytes()
    return (out.numpy(np.int64, NC, max_out), img.numpy(np.int64, NI), None if emap is None else emap.numpy(np.uint8, h, w),
            None if smap is None else smap.numpy(np.uint8, h, w))


def assert_equals_host(got, lab, p, thresh, band, lo=None, hi=None, max_out=MAX_OUT):
    want = dc.confidence_numpy(lab, p, thresh, band, lo, hi, max_out=max_out, maps=True)
    rows, image, emap, smap = got
    for j, name in enumerate(dc.CONF_QUANTITIES):
        assert np.array_equal(rows[j], want[name]), name
    assert np.array_equal(image, want["image"]), (image, want["image"])
    if emap is not None:
        assert np.array_equal(emap, want["entropy_u8"])
    if smap is not None:
        assert np.array_equal(smap, want["spread_u8"])
    return want


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("envelope,maps", [(False, False), (True, True), (True, False), (False, True)])
def test_fixtures_equal_the_host_path(geometry, envelope, maps):
    lab, p, lo, hi = fixture(*geometry)
    env = (lo, hi) if envelope else (None, None)
    got = device_confidence(lab, p, THRESH, BAND, *env, maps=maps)
    want = assert_equals_host(got, lab, p, THRESH, BAND, *env)
    if geometry == (96, 130, 96, 130):                       # the runs of p = 1.0: 130 and 64 pixels of q^2 = 65535^2
        assert want["Sqq"][1] >= 130 * 65535 ** 2 > 2 ** 38 and want["Sqq"][2] >= 64 * 65535 ** 2
    again = device_confidence(lab, p, THRESH, BAND, *env, maps=maps)
    for a, b in zip(got, again):                             # two calls, the same bytes
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


@pytest.mark.parametrize("band", [0.0, 0.5])
def test_band_limits(band):
    lab, p, lo, hi = fixture(96, 130, 64, 64)
    assert_equals_host(device_confidence(lab, p, 0.5, band, lo, hi, maps=True), lab, p, 0.5, band, lo, hi)


def test_past_the_grid_cap():
    """1500 x 1500 random labels: 36000 wave units on a grid capped at 2048 workgroups of four, so the grid-stride loop runs; a
    512 x 512 plane underneath (the flow's kind of resize)."""
    rng = np.random.default_rng(15)
    lab = rng.integers(-1, 41, (1500, 1500)).astype(np.int32)
    p, lo, hi = planes(512, 512, seed=15)
    assert_equals_host(device_confidence(lab, p, THRESH, BAND, lo, hi, max_out=32, maps=True), lab, p, THRESH, BAND, lo, hi, max_out=32)


def test_no_capacity_and_stale_outputs():
    lab, p, lo, hi = fixture(37, 53, 16, 16)
    rows, image, _, _ = device_confidence(lab, p, THRESH, BAND, lo, hi, max_out=0, null_out=True)
    want = dc.confidence_numpy(lab, p, THRESH, BAND, lo, hi, max_out=0)
    assert rows.size == 0 and np.array_equal(image, want["image"]) and image[1] == int((lab > 0).sum()) > 0
    old = device_confidence(label_map(37, 53, seed=99), planes(16, 16, seed=98)[0], 0.6, 0.2, max_out=MAX_OUT)
    for prefill in (0xFF, 0x00, (old[0], old[1])):
        assert_equals_host(device_confidence(lab, p, THRESH, BAND, lo, hi, prefill=prefill), lab, p, THRESH, BAND, lo, hi)
        assert_equals_host(device_confidence(lab, p, THRESH, BAND, prefill=prefill), lab, p, THRESH, BAND)


def test_refusals_come_before_any_launch():
    """Host memory stands in for device memory: every call below must return UNETDC_EINVAL without touching it."""
    from unet_dc_segmentation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) // 64 * 64

    def call(label=a, max_out=4, h=8, w=8, probs=a, lo=None, hi=None, ph=8, pw=8, band=0.1, table=a, out=a, image=a, emap=None, smap=None):
        return lib.unetdc_label_confidence(label, max_out, h, w, probs, lo, hi, ph, pw, 0.5, band, table, out, image, emap, smap, None)
    cases = [(dict(lo=a), b"envelope"), (dict(hi=a), b"envelope"), (dict(smap=a), b"spread map"), (dict(h=0), b"geometry"),
             (dict(w=16385), b"geometry"), (dict(h=-1), b"geometry"), (dict(h=16384, w=16384 * 4), b"geometry"), (dict(ph=0), b"geometry"),
             (dict(pw=0), b"geometry"), (dict(max_out=-1), b"geometry"), (dict(h=2 ** 15, w=2 ** 15), b"geometry"),
             (dict(image=None), b"null"), (dict(out=None), b"null"), (dict(table=None), b"null"), (dict(probs=None), b"null"),
             (dict(label=None), b"null"), (dict(band=0.6), b"band"), (dict(band=-0.1), b"band"), (dict(band=float("nan")), b"band")]
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.unetdc_last_error()
        assert rc == -1 and err.startswith(b"label_confidence") and msg in err, (kw, rc, err)
    assert bytes(buf.raw) == bytes(4096)
    p = a + 1024
    for args, msg in (((a, 1, 16, 2, p, None, p + 1024), b"null"), ((a, 1, 16, 2, p + 4, p + 1024, p + 2048), b"aligned"),
                      ((a, 1, 16, 2, p, p + 1024 + 8, p + 2048), b"aligned"), ((a, 1, 16, 2, a + 2048 - 16, p + 1024, p + 2048), b"overlap"),
                      ((a, 1, 16, 2, p + 1024, p, p + 2048), b"overlap"), ((a, 1, 16, 2, p + 1024, p + 2048, p + 1024 + 512), b"overlap"),
                      ((a, 1, 24, 2, p, p, p), b"plane size"), ((a, 1, 16, 3, p, p, p), b"variants")):
        rc = lib.unetdc_dihedral_mean_env_f32(*args, None)
        err = lib.unetdc_last_error()
        assert rc == -1 and err.startswith(b"dihedral_mean_env") and msg in err, (args, rc, err)
    assert bytes(buf.raw) == bytes(4096)


# ---- the envelope kernel -----------------------------------------------------------------------------------------------------------

def mean_env_abi(p, N):
    from unet_dc_segmentation_amd import _lib
    s, n = p.shape[-1], p.shape[0] // N
    src = canaried_like(p, align=16)
    outs = [Canaried(n * s * s * 4, align=16) for _ in range(3)]
    _lib.call("unetdc_dihedral_mean_env_f32", src.ptr, n, s, N, *(o.ptr for o in outs), _stream())
    torch.cuda.synchronize()
    for o in (src, *outs):
        o.check()
    assert src.numpy(np.uint32, *p.shape).tobytes() == p.tobytes()
    return [o.numpy(np.float32, n, s, s) for o in outs]


@pytest.mark.parametrize("N", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("s", [16, 32, 48])
def test_mean_env_equals_the_mean_kernel_and_numpy(s, n, N):
    from tests.test_gpu_tta import mean_abi
    p = np.random.default_rng(s * 100 + n * 10 + N).random((n * N, s, s), dtype=np.float32)
    mean, lo, hi = mean_env_abi(p, N)
    assert mean.tobytes() == mean_abi(p, N).tobytes()
    want = tta.mean_env_numpy(p, N)
    for got, ref in zip((mean, lo, hi), want):
        assert got.tobytes() == ref.tobytes()


def test_mean_env_past_the_grid_cap():
    """9 images of 512 x 512, N = 2: 9216 output blocks = 2304 trips of four on a grid capped at 2048 workgroups."""
    from unet_dc_segmentation_amd.tta import dihedral_mean, dihedral_mean_env
    p = np.random.default_rng(4).random((18, 512, 512), dtype=np.float32)
    d = torch.from_numpy(p).cuda()
    got = dihedral_mean_env(d, 2)
    assert torch.equal(got[0], dihedral_mean(d, 2))
    for g, ref in zip(got, tta.mean_env_numpy(p, 2)):
        assert g.cpu().numpy().tobytes() == ref.tobytes()
    outs = tuple(torch.empty(9, 512, 512, device="cuda") for _ in range(3))
    assert all(a is b for a, b in zip(dihedral_mean_env(d, 2, out=outs), outs)) and torch.equal(outs[2], got[2])
    from unet_dc_segmentation_amd import _lib
    for bad in (lambda: dihedral_mean_env(d, 3), lambda: dihedral_mean_env(d[:17], 2), lambda: dihedral_mean_env(d, 2, out=outs[:2]),
                lambda: dihedral_mean_env(d, 2, out=(outs[0], outs[0], outs[1])), lambda: dihedral_mean_env(p, 2)):
        with pytest.raises(_lib.UnetdcError):
            bad()


# ---- droplets.py -------------------------------------------------------------------------------------------------------------------

def batch_inputs():
    from tests.test_split_cpu import noise_mask
    hws = [(120, 160), (97, 131), (64, 80)]
    rng = np.random.default_rng(31)
    p = np.stack([np.where(noise_mask(64, 80, seed=70 + i, sigma=2.0, frac=0.35) > 0, 0.55, 0.1).astype(np.float32) for i in range(3)])
    p = (p + rng.random(p.shape, dtype=np.float32) * np.float32(0.4)).astype(np.float32)
    lo = (p - rng.random(p.shape, dtype=np.float32) * np.float32(0.2)).astype(np.float32)
    hi = (p + rng.random(p.shape, dtype=np.float32) * np.float32(0.2)).astype(np.float32)
    return hws, p, lo, hi


def assert_record_equals_host(d, p, thresh, band, lo=None, hi=None, maps=False):
    lab = d.labels.cpu().numpy()
    want = dc.confidence_numpy(lab, p, thresh, band, lo, hi, max_out=len(d.area), maps=True)
    rec = d.confidence
    for name in dc.CONF_QUANTITIES:
        assert rec[name].dtype == np.int64 and np.array_equal(rec[name], want[name]), name
    assert rec["image"].dtype == np.int64 and np.array_equal(rec["image"], want["image"]) and rec["envelope"] == (lo is not None)
    assert np.array_equal(rec["n"], d.area)
    for key in ("entropy_u8", "spread_u8"):
        if maps and want[key] is not None:
            assert rec[key].is_cuda and np.array_equal(rec[key].cpu().numpy(), want[key])
        else:
            assert rec[key] is None
    cols, ref = dc.confidence_columns(rec), dc.confidence_columns(want)
    assert list(cols) == list(ref) and all(np.array_equal(cols[k], ref[k]) for k in ref)
    assert str(dc.image_columns(rec)) == str(dc.image_columns(want))             # as text: a NaN equals a NaN


@pytest.mark.parametrize("kw", [dict(), dict(split_depth=1.0), dict(shape=True, neighbors=3), dict(max_hole_area=-1, thresh_low=0.45)])
def test_through_mask_and_droplets_batch(kw):
    from unet_dc_segmentation_amd import droplets as D
    hws, p, lo, hi = batch_inputs()
    probs, env = torch.from_numpy(p).cuda(), (torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda())
    before = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, **(kw if "split_depth" in kw else dict(kw, shape=True)))
    out = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, confidence=0.1, confidence_maps=True, envelope=env, **kw)
    assert min(len(d.area) for d in out) > 4
    for i, (d, b) in enumerate(zip(out, before)):
        assert_record_equals_host(d, p[i], 0.5, 0.1, lo[i], hi[i], maps=True)
        assert b.confidence is None and torch.equal(d.mask, b.mask) and torch.equal(d.labels, b.labels) and np.array_equal(d.area, b.area)
        assert np.array_equal(d.centroid_row, b.centroid_row) and np.array_equal(d.clean_counts, b.clean_counts)
    plain = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, confidence=0.25, **kw)
    for i, d in enumerate(plain):
        assert_record_equals_host(d, p[i], 0.5, 0.25)
    # fewer output slots than droplets: the re-run carries the option and the envelope through
    again = D.mask_and_droplets_batch(probs, 0.5, hws, 2, max_droplets=4, return_labels=True, confidence=0.1, envelope=env, **kw)
    for d, a in zip(out, again):
        assert all(np.array_equal(d.confidence[k], a.confidence[k]) for k in dc.CONF_QUANTITIES + ("image",)) and a.confidence["envelope"]
    one = D.mask_and_droplets(probs[1], 0.5, hws[1], 2, confidence=0.1, envelope=(env[0][1], env[1][1]), **kw)
    assert one.labels is None and all(np.array_equal(one.confidence[k], out[1].confidence[k]) for k in dc.CONF_QUANTITIES + ("image",))
    with pytest.raises(D._lib.UnetdcError):
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, envelope=env)
    with pytest.raises(D._lib.UnetdcError):
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, confidence=0.1, envelope=(env[0], env[1][:, :32]))


def test_the_option_adds_no_copy_and_no_wait(monkeypatch):
    from unet_dc_segmentation_amd import droplets as D
    hws, p, lo, hi = batch_inputs()
    probs, env = torch.from_numpy(p).cuda(), (torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda())
    calls = {"cpu": 0, "names": []}
    real_cpu, real_call = torch.Tensor.cpu, D._lib.call

    def cpu(self, *a, **k):
        calls["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)

    def call(name, *a):
        calls["names"].append(name)
        return real_call(name, *a)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", cpu)
        mp.setattr(D._lib, "call", call)
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, shape=True)
        off = list(calls["names"])
        assert calls["cpu"] == 3 and "unetdc_label_confidence" not in off
        calls.update(cpu=0, names=[])
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, shape=True, confidence=0.1, confidence_maps=True, envelope=env)
        assert calls["cpu"] == 3
        assert [n for n in calls["names"] if n != "unetdc_label_confidence"] == off and calls["names"].count("unetdc_label_confidence") == 3


# ---- the script ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,args,sizes", [
    ("plain", ["--confidence", "--confidence_maps"], ((96, 96), (80, 112), (64, 64))),
    ("tta4", ["--confidence", "0.2", "--tta", "4", "--confidence_maps"], ((96, 96), (80, 112), (64, 64))),
    ("tiled", ["--confidence", "--tta", "2", "--tile", "64", "--tile_overlap", "16"], ((96, 130),))])
def test_cli_device_equals_cpu_path(tmp_path, monkeypatch, tag, args, sizes):
    """quantify_droplets_batch.py --confidence on the device against its CPU path on the synthetic set: the network is the exact
    stand-in of tests/test_tta_cpu.py, so the probabilities, the envelope and with them every integer agree; the float columns
    are the same float64 formulas on equal integers."""
    import pandas as pd
    import quantify_droplets_batch as q
    from tests.test_confidence_cpu import files
    assert q.DEVICE == "cuda"
    dev = run_script(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes)
    cpu = run_script(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes)
    assert files(dev) == files(cpu) and "confidence_per_image.csv" in files(dev)
    for f in files(dev):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    t = pd.read_csv(dev / "all_droplets.csv")
    assert len(t) > 3 and t["prob_mean"].notna().all() and ("--tta" in args) == ("tta_spread_mean" in t.columns)
