"""GPU: the threshold sweep (unetdc_thresh_sweep, csrc/sweep.hip) through the C ABI against the host
path of the same definition (utils/threshold_sweep.py, itself pinned to tests/sweep_ref.py on the CPU) and against the
library's own mask kernels launched once per threshold; then evaluate.py, the script's flags and --calibrate_thresh.
Integer work: bit-exact."""
import functools

import numpy as np
import pytest
import torch

from tests.test_sweep_cpu import GEOMETRIES, TRAIN_ARGS, edge_probs, gt_of
from utils import threshold_sweep as ts

pytestmark = pytest.mark.gpu

GUARD = 256                     # int64 words on both sides of the histogram
CANARY64 = -0x5A5A5A5A5A5A5A5B


def stream():
    return torch.cuda.current_stream().cuda_stream


def tables(ph, pw, oh, ow):
    from unet_dc_segmentation_amd.preprocess import _resize_tables
    xo, xa = _resize_tables(pw, ow, "cuda", True)
    yo, ya = _resize_tables(ph, oh, "cuda", False)
    return [xo, xa, yo, ya]


def device_sweep(probs, gt, K, linear, into=None):
    """probs [n][ph][pw] fp32, gt [n][oh][ow] uint8 (numpy or device tensors) -> int64 [2][K + 1].  The histogram starts at
    `into` (zeros without) and sits between GUARD canary words on both sides, which the call must leave alone."""
    from unet_dc_segmentation_amd import _lib
    p = (probs if torch.is_tensor(probs) else torch.from_numpy(np.array(probs, dtype=np.float32))).cuda()
    g = (gt if torch.is_tensor(gt) else torch.from_numpy(np.array(gt, dtype=np.uint8))).cuda()
    n, ph, pw = p.shape
    oh, ow = g.shape[1:]
    nb = 2 * (K + 1)
    buf = torch.full((nb + 2 * GUARD,), CANARY64, dtype=torch.int64, device="cuda")
    buf[GUARD:GUARD + nb] = 0 if into is None else torch.from_numpy(np.asarray(into, np.int64).reshape(-1)).cuda()
    tb = tables(ph, pw, oh, ow) if linear else [None] * 4
    _lib.call("unetdc_thresh_sweep", p.data_ptr(), n, ph, pw, g.data_ptr(), oh, ow, *(None if t is None else t.data_ptr() for t in tb),
              K, buf[GUARD:].data_ptr(), stream())
    b = buf.cpu().numpy()
    assert np.all(b[:GUARD] == CANARY64) and np.all(b[GUARD + nb:] == CANARY64), "write outside the histogram"
    return b[GUARD:GUARD + nb].reshape(2, K + 1)


@functools.lru_cache(maxsize=None)
def fixture(name, K):
    """(probs [3][ph][pw], gt [3][oh][ow], the host path's histogram per image) of a geometry; computed once, read-only."""
    _, (ph, pw), (oh, ow), linear = next(geo for geo in GEOMETRIES if geo[0] == name)
    p, g = edge_probs(ph, pw, K, seed=K, n=3), gt_of(oh, ow, seed=K, n=3)
    hists = np.stack([ts.sweep_hist_numpy(p[i], g[i], (oh, ow), K, linear=linear) for i in range(3)])
    for a in (p, g, hists):
        a.setflags(write=False)
    return p, g, hists


@pytest.mark.parametrize("K", (1, 10, 100, 1024))
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_device_equals_host_path(geo, K):
    name, _, (oh, ow), linear = geo
    p, g, hists = fixture(name, K)
    h = device_sweep(p, g, K, linear)
    assert h.sum() == 3 * oh * ow and np.array_equal(h, hists.sum(axis=0))
    assert np.array_equal(device_sweep(p[1:2], g[1:2], K, linear), hists[1])          # one image of the batch on its own


def masks_by_the_library(p, oh, ow, K, linear, ks=None):
    """[len(ks)][oh][ow] bool: unetdc_mask_from_probs[_linear] launched once per threshold k / K, k in ks (all without)."""
    from unet_dc_segmentation_amd import _lib
    ph, pw = p.shape
    pd = torch.from_numpy(np.ascontiguousarray(p)).cuda()
    ks = range(K) if ks is None else ks
    out = torch.empty(len(ks), oh, ow, dtype=torch.uint8, device="cuda")
    tb = tables(ph, pw, oh, ow) if linear else None
    for k, t in enumerate(ts.grid(K)[list(ks)]):
        if linear:
            _lib.call("unetdc_mask_from_probs_linear", pd.data_ptr(), ph, pw, float(t), out[k].data_ptr(), oh, ow,
                      *(x.data_ptr() for x in tb), stream())
        else:
            _lib.call("unetdc_mask_from_probs", pd.data_ptr(), ph, pw, float(t), out[k].data_ptr(), oh, ow, stream())
    return out != 0


@pytest.mark.parametrize("case", [("linear_aniso", (64, 64), (130, 173), 100, True), ("full_size", (512, 512), (1040, 1388), 10, True),
                                  ("nearest_down", (40, 40), (17, 23), 100, False)], ids=lambda c: c[0])
def test_tail_sums_equal_the_mask_kernels_launched_k_times(case):
    _, (ph, pw), (oh, ow), K, linear = case
    p, g = edge_probs(ph, pw, K, seed=5)[0], gt_of(oh, ow, seed=5)[0]
    h = device_sweep(p[None], g[None], K, linear)
    m = masks_by_the_library(p, oh, ow, K, linear)
    gd = torch.from_numpy(g != 0).cuda()
    tp = (m & gd).sum(dim=(1, 2)).cpu().numpy()
    fp = (m & ~gd).sum(dim=(1, 2)).cpu().numpy()
    tail = h[:, ::-1].cumsum(axis=1)[:, ::-1]
    assert np.array_equal(tail[1, 1:], tp) and np.array_equal(tail[0, 1:], fp) and tp[0] > 0 and fp[0] > 0
    table = ts.sweep_table(h)
    assert np.array_equal(table["tp"], tp) and np.array_equal(table["fp"], fp)


def test_past_the_grid_cap_and_under_contention():
    oh, ow = 1040, 1388
    zero = torch.zeros(1, 512, 512, device="cuda")
    h = device_sweep(zero, torch.zeros(1, oh, ow, dtype=torch.uint8, device="cuda"), 1024, True)
    assert h[0, 0] == oh * ow and h.sum() == oh * ow              # every lane of every wave in one bin
    h = device_sweep(zero, torch.ones(1, oh, ow, dtype=torch.uint8, device="cuda"), 100, False)
    assert h[1, 0] == oh * ow and h.sum() == oh * ow
    # a ramp over the source columns: every level 0..1024 occurs, and the identity geometry gives each its exact count
    K = 1024
    g = ts.grid(K)
    ramp = np.concatenate([g, np.nextafter(g, np.float32(2)), [np.float32(1.0)]]).astype(np.float32)     # 2049 values
    p = np.resize(ramp, (1, oh, ow)).astype(np.float32)
    gt = (np.arange(oh * ow).reshape(1, oh, ow) % 5 == 0).astype(np.uint8)      # 5 and 2049 are coprime: every pair occurs
    h = device_sweep(p, gt, K, False)
    lev = np.searchsorted(g, p.ravel(), side="left")               # #{k: t_k < p}
    want = np.bincount(gt.ravel().astype(np.int64) * (K + 1) + lev, minlength=2 * (K + 1)).reshape(2, K + 1)
    assert np.array_equal(h, want) and (h > 0).all()
    p512 = np.resize(ramp, (512, 512)).astype(np.float32)          # and through the linear rule, against single mask launches
    hl = device_sweep(p512[None], gt, K, True)
    ks = (0, 1, 300, 512, 1023)
    m = masks_by_the_library(p512, oh, ow, K, True, ks).sum(dim=(1, 2)).cpu().numpy()
    assert hl.sum() == oh * ow and [int(hl[:, k + 1:].sum()) for k in ks] == m.tolist() and m[-1] > 0


def test_calls_accumulate_and_two_runs_are_bitwise_equal():
    name, _, _, linear = GEOMETRIES[3]
    p, g, hists = fixture(name, 100)
    a = device_sweep(p[:1], g[:1], 100, linear)
    both = device_sweep(p[1:], g[1:], 100, linear, into=a)
    assert np.array_equal(a, hists[0]) and np.array_equal(both, hists.sum(axis=0))
    assert device_sweep(p, g, 100, linear).tobytes() == device_sweep(p, g, 100, linear).tobytes() == both.tobytes()
    big = np.full((2, 101), 1 << 40, np.int64)                      # the adds are 64-bit
    assert np.array_equal(device_sweep(p, g, 100, linear, into=big), both + (1 << 40))


def test_a_short_grid_writes_four_entries():
    p = np.array([[[0.0, 0.5], [np.nan, 1e-45]]], np.float32)
    g = np.array([[[1, 0], [0, 9]]], np.uint8)
    assert device_sweep(p, g, 1, False).tolist() == [[1, 1], [1, 1]]       # the guards of device_sweep start right behind


def test_refusals_leave_the_histogram_alone():
    from unet_dc_segmentation_amd import _lib
    lib = _lib.load()
    p = torch.rand(1, 8, 8, device="cuda")
    g = torch.ones(1, 8, 8, dtype=torch.uint8, device="cuda")
    tb = [t.data_ptr() for t in tables(8, 8, 8, 8)]
    hist = torch.full((2 * 1025 + GUARD,), CANARY64, dtype=torch.int64, device="cuda")
    ok = dict(probs=p.data_ptr(), n=1, ph=8, pw=8, gt=g.data_ptr(), oh=8, ow=8, tb=[None] * 4, k=10, hist=hist.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return lib.unetdc_thresh_sweep(a["probs"], a["n"], a["ph"], a["pw"], a["gt"], a["oh"], a["ow"], *a["tb"], a["k"], a["hist"],
                                       stream())
    bad = [dict(probs=None), dict(gt=None), dict(hist=None), dict(k=0), dict(k=1025), dict(k=-1), dict(n=0), dict(n=-2),
           dict(ph=0), dict(pw=0), dict(oh=0), dict(ow=0), dict(ph=16385), dict(pw=16385), dict(oh=16385), dict(ow=16385)]
    bad += [dict(tb=[None if j == i else tb[j] for j in range(4)]) for i in range(4)] + [dict(tb=[tb[0], None, None, None])]
    for kw in bad:
        assert call(**kw) == -1 and lib.unetdc_last_error(), kw
    torch.cuda.synchronize()
    assert bool((hist == CANARY64).all())
    hist.zero_()
    assert call() == 0 and call(tb=tb) == 0                         # the same arguments, accepted: both rules at identity size
    assert int(hist[:22].sum()) == 128 and int(hist[22:].sum()) == 0


def test_sweep_batch_with_mixed_sizes_equals_single_images_and_copies_once(monkeypatch):
    from unet_dc_segmentation_amd.evaluate import sweep_batch, sweep_result
    sizes = [(130, 173), (130, 173), (64, 64), (97, 33), (130, 173)]
    K = 100
    p = edge_probs(64, 64, K, seed=3, n=len(sizes))
    gts = [gt_of(h, w, seed=20 + i)[0] for i, (h, w) in enumerate(sizes)]
    gts[3] = gts[3].astype(np.int32) * 300                          # a label image: any nonzero value is annotated
    probs = torch.from_numpy(p).cuda()
    calls = {"cpu": 0, "item": 0, "sync": 0}
    real_cpu, real_item, real_sync = torch.Tensor.cpu, torch.Tensor.item, torch.cuda.synchronize

    def cpu(self, *a, **k):
        calls["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)

    def item(self):
        calls["item"] += self.is_cuda
        return real_item(self)

    def sync(*a, **k):
        calls["sync"] += 1
        return real_sync(*a, **k)
    from unet_dc_segmentation_amd import _lib
    _lib.start_timing(["unetdc_thresh_sweep"])
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", cpu)
        mp.setattr(torch.Tensor, "item", item)
        mp.setattr(torch.cuda, "synchronize", sync)
        hist = sweep_batch(probs[:3], gts[:3], sizes[:3], K)
        hist = sweep_batch(probs[3:], gts[3:], sizes[3:], K, hist=hist)     # a second batch pools into the same histogram
        assert calls == {"cpu": 0, "item": 0, "sync": 0}
        out = sweep_result(hist)
        assert calls == {"cpu": 1, "item": 0, "sync": 0}
    recs = _lib.stop_timing()
    assert [r[1][1] for r in recs] == [2, 1, 1, 1]                  # the run of two equal sizes is ONE call
    want = sum(ts.sweep_hist_numpy(p[i], gts[i], sizes[i], K) for i in range(len(sizes)))
    assert out.dtype == np.int64 and np.array_equal(out, want)
    single = sum(sweep_result(sweep_batch(probs[i:i + 1], gts[i:i + 1], sizes[i:i + 1], K)) for i in range(len(sizes)))
    assert np.array_equal(single, out)
    near = sweep_result(sweep_batch(probs[:2], gts[:2], sizes[:2], K, linear=False))
    assert np.array_equal(near, sum(ts.sweep_hist_numpy(p[i], gts[i], sizes[i], K, linear=False) for i in range(2)))
    with pytest.raises(_lib.UnetdcError):
        sweep_batch(probs[:1], gts[:1], sizes[:1], K, hist=torch.zeros(2, K, dtype=torch.int64, device="cuda"))


def cli_fixture(tmp_path):
    from PIL import Image
    from tests.test_split_cpu import noise_mask
    sizes = ((512, 512), (300, 401), (1040, 1388), (96, 130), (512, 512))
    rng = np.random.default_rng(7)
    masks = [noise_mask(512, 512, seed=60 + i, sigma=4.0, frac=0.4) for i in range(len(sizes))]
    # graded probabilities: blobs at 0.55..0.95, background at 0.05..0.45, so that every threshold of the grid cuts differently
    p = np.stack([np.where(m > 0, 0.55, 0.05) + 0.4 * rng.random((512, 512)) for m in masks]).astype(np.float32)
    p[4] = 0.1
    gt_dir = tmp_path / "gt"
    if not gt_dir.exists():
        gt_dir.mkdir()
        for i, (h, w) in enumerate(sizes):
            Image.fromarray(noise_mask(h, w, seed=80 + i, sigma=4.0, frac=0.3) * 255).save(gt_dir / f"im{i}.png")
    return sizes, torch.from_numpy(p)[:, None], gt_dir


@pytest.mark.parametrize("extra", [[], ["--split_touching", "--prob_thresh_low", "0.3", "--fill_holes", "20"]],
                         ids=["plain", "split_and_clean"])
def test_cli_sweep_device_equals_cpu_path(tmp_path, monkeypatch, extra):
    import pandas as pd
    from PIL import Image
    import quantify_droplets_batch as q
    from tests.test_split_cpu import files, run_cli
    assert q.DEVICE == "cuda"
    sizes, probs, gt_dir = cli_fixture(tmp_path)
    args = ["--min_area", "3", "--gt_dir", str(gt_dir), "--gt_min_area", "4", "--thresh_sweep", "10", "--sweep_objects", "0.5,0.7"] + extra
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    assert files(dev) == files(cpu) and {"threshold_sweep.csv", "threshold_sweep_objects.csv"} <= set(files(dev))
    for f in ("threshold_sweep.csv", "threshold_sweep_objects.csv", "match_per_image.csv"):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    o = pd.read_csv(dev / "threshold_sweep_objects.csv", float_precision="round_trip")
    m = pd.read_csv(dev / "match_per_image.csv", float_precision="round_trip")
    assert o["threshold"].tolist() == [0.5, 0.7] and list(o.columns)[1:] == list(m.columns)[1:]
    ints = [c for c in m.columns if m[c].dtype.kind == "i"]
    assert len(ints) >= 19 and o.loc[0, ints].tolist() == m.loc[m["filename"] == "ALL", ints].iloc[0].tolist()
    assert o["n_pred"][0] > 20 and o["n_pred"][1] != o["n_pred"][0]
    t = pd.read_csv(dev / "threshold_sweep.csv", float_precision="round_trip")
    assert len(t) == 10 and (t["tp"] + t["fp"] + t["fn"] + t["tn"] == sum(h * w for h, w in sizes)).all()
    if not extra:                                                  # the raw mask at --prob_thresh is the mask the run wrote
        row = t[t["threshold"].astype(np.float32) == np.float32(0.5)]
        px = sum(int((np.array(Image.open(dev / "predicted_masks" / f"im{i}_pred.png")) > 0).sum()) for i in range(len(sizes)))
        assert len(row) == 1 and int(row["tp"].iloc[0] + row["fp"].iloc[0]) == px > 0


def test_cli_without_the_flags_launches_nothing_new(tmp_path, monkeypatch):
    from unet_dc_segmentation_amd import _lib
    from tests.test_split_cpu import files, run_cli
    sizes, probs, gt_dir = cli_fixture(tmp_path)
    args = ["--min_area", "3", "--gt_dir", str(gt_dir), "--gt_min_area", "4"]
    _lib.start_timing(_lib.SIGNATURES)
    plain = run_cli(tmp_path, monkeypatch, "plain", args, device="cuda", sizes=sizes, probs=probs)
    names = {r[0].split("|")[0] for r in _lib.stop_timing()}
    assert "unetdc_thresh_sweep" not in names and {"unetdc_label_overlap", "unetdc_mask_from_probs_linear"} <= names
    _lib.start_timing(_lib.SIGNATURES)
    swept = run_cli(tmp_path, monkeypatch, "swept", args + ["--thresh_sweep"], device="cuda", sizes=sizes, probs=probs)
    recs = _lib.stop_timing()
    assert sum(r[0].split("|")[0] == "unetdc_thresh_sweep" for r in recs) == 5          # one per image: every size differs from its neighbour
    assert sorted(set(files(swept)) - set(files(plain))) == ["threshold_sweep.csv"]
    expected = {"summary_per_image.csv", "all_droplets.csv", "droplet_size_stats.csv", "gt_droplets.csv", "match_per_image.csv"}
    expected |= {f"im{i}_droplets.csv" for i in range(5)} | {f"predicted_masks/im{i}_pred.png" for i in range(5)}
    assert set(files(plain)) == expected
    for f in files(plain):
        assert (plain / f).read_bytes() == (swept / f).read_bytes(), f


def test_calibrate_thresh_on_the_device(tmp_path, monkeypatch):
    """history.calibration["hist"] is the host path's histogram of the probabilities the model gave in its last pass over the
    validation split (captured at the model's forward) and of that split's masks."""
    import train_DC_focal as t
    from models.model_2 import UNetDC
    seen = []
    real = UNetDC.forward

    def forward(self, x):
        y = real(self, x)
        if not self.training:
            seen.append(y.detach().float().cpu().numpy())
        return y
    monkeypatch.setattr(UNetDC, "forward", forward)
    argv = [a for a in TRAIN_ARGS if a not in ("--device", "cpu")] + ["--ckpt_path", str(tmp_path / "ck.pth")]
    hist = t.main(argv + ["--calibrate_thresh", "100"])
    c = hist.calibration
    val = t.make_datasets(t.build_parser().parse_args(argv))[1]
    assert len(val) == 2 and c["K"] == 100 and c["hist"].shape == (2, 101) and c["hist"].sum() == 2 * 32 * 32
    probs = seen[-1]                                                # batch 2 = the whole validation split, the last eval pass
    assert probs.shape == (2, 1, 32, 32)
    want = sum(ts.sweep_hist_numpy(probs[i, 0], (val[i][1][0].numpy() > 0.5), (32, 32), 100, linear=False) for i in range(2))
    assert np.array_equal(c["hist"], want)
    table = ts.sweep_table(want)
    assert c["best_dice"] == table["dice"].max() and c["best_dice_threshold"] == table["threshold"][table["best_dice_k"]]
    assert c["average_precision"] == table["average_precision"]
    seen.clear()
    assert t.main(argv).calibration is None
