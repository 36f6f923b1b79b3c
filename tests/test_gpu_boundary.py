"""GPU: surface distances (unetdc_boundary_distances, csrc/boundary.hip) through the C ABI against the host path of the same
definition (utils/droplet_boundary.py, itself pinned to the plain loops of tests/boundary_ref.py on the CPU); then evaluate.py,
the CLI flag and the training script's report.  Integer work: bit-exact."""
import functools

import numpy as np
import pytest
import torch

from tests import workspace_states as wstates
from tests.image_canaries import Canaried
from tests.test_gpu_split import probs_of, stream
from tests.test_match_cpu import big_pair, small_pairs
from tests.test_split_cpu import noise_mask
from utils import droplet_boundary as db

pytestmark = pytest.mark.gpu

RADII = (1, 3, 64)
KEYS = ("hist", "dmax", "a", "b")


def device_boundary(A, ka, B, kb, R, ws=None, into=None, tables=(True, True)):
    """-> the record as int64 numpy arrays (a / b None where no table was passed).  hist, dmax, the two tables and the workspace
    sit between canaries; the tables start as canary bytes, so an entry the call did not initialise shows.  into: (hist, dmax)
    Canaried views of an earlier call to add into; ws: a prepared Canaried view of exactly the queried bytes."""
    from unet_dc_segmentation_amd import _lib
    A, B = np.ascontiguousarray(A, dtype=np.int32), np.ascontiguousarray(B, dtype=np.int32)
    h, w = A.shape
    nb = R * R + 2
    lib = _lib.load()
    nbytes = lib.unetdc_boundary_distances_workspace(h, w)
    assert nbytes == 10 * h * w + 64
    ws = Canaried(nbytes) if ws is None else ws
    assert ws.nbytes == nbytes
    if into is None:
        hist, dmax = Canaried(2 * nb * 8), Canaried(8)
        hist.u8.zero_()
        dmax.u8.fill_(0xFF)                                    # two int32 of -1
    else:
        hist, dmax = into
    ta = Canaried(3 * ka * 8) if tables[0] and ka else None
    tb = Canaried(3 * kb * 8) if tables[1] and kb else None
    da, dbb = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B.copy()).cuda()
    _lib.call("unetdc_boundary_distances", da.data_ptr(), ka, dbb.data_ptr(), kb, h, w, R, ws.ptr, nbytes, hist.ptr, dmax.ptr,
              ta.ptr if ta else None, tb.ptr if tb else None, stream())
    for v, what in ((ws, "workspace"), (hist, "hist"), (dmax, "dmax"), (ta, "table a"), (tb, "table b")):
        if v is not None:
            v.check(what)
    assert np.array_equal(da.cpu().numpy(), A) and np.array_equal(dbb.cpu().numpy(), B)       # the inputs are read only
    empty = {True: np.zeros((3, 0), np.int64), False: None}
    return {"hist": hist.numpy(np.int64, 2, nb).copy(), "dmax": dmax.numpy(np.int32, 2).astype(np.int64),
            "a": ta.numpy(np.int64, 3, ka).copy() if ta else empty[tables[0]],
            "b": tb.numpy(np.int64, 3, kb).copy() if tb else empty[tables[1]], "views": (hist, dmax)}


@functools.lru_cache(maxsize=None)
def host_record(name, R, big=False):
    A, ka, B, kb = big_pair(name) if big else small_pairs()[name]
    return db.boundary_record_numpy(A, ka, B, kb, R)


def assert_same(got, want, what=""):
    for q in KEYS:
        if want[q] is None:
            assert got[q] is None, (what, q)
        else:
            assert got[q].shape == want[q].shape and np.array_equal(got[q], want[q]), (what, q, got[q], want[q])


@pytest.mark.parametrize("name", sorted(small_pairs()))
def test_small_pairs_equal_the_host_path(name):
    """Wave-edge widths 63 / 64 / 65, 1 x 1, 1 x 65, 3 x 1388, the checkerboard where every pixel is boundary, vs_zeros (INF)."""
    A, ka, B, kb = small_pairs()[name]
    for R in RADII:
        assert_same(device_boundary(A, ka, B, kb, R), host_record(name, R), (name, R))
    if name.endswith("vs_zeros") and ka:
        assert host_record(name, 64)["dmax"].tolist() == [db.EDT_INF, -1]
    if name == "checkerboard":
        assert host_record(name, 3)["hist"].sum(1).tolist() == [21 * 130, 21 * 130]


@pytest.mark.parametrize("name", ["noise9_vs_shifted", "one_vs_noise21"])
def test_full_size_pairs_twice(name):
    """1040 x 1388.  one_vs_noise21: few query pixels on one side, 100 k far pixels on the other -- the long scans."""
    A, ka, B, kb = big_pair(name)
    want = host_record(name, 64, True)
    one = device_boundary(A, ka, B, kb, 64)
    assert_same(one, want, name)
    two = device_boundary(A, ka, B, kb, 64)
    for q in KEYS:
        assert one[q].tobytes() == two[q].tobytes(), q
    far = int(want["hist"][:, -1].sum())
    assert far == (100482 if name == "one_vs_noise21" else 0)


def test_the_call_adds_and_pools():
    p = small_pairs()
    one, two = p["37x53/cc_vs_shifted"], p["37x53/split_vs_cc"]
    w1, w2 = host_record("37x53/cc_vs_shifted", 3), host_record("37x53/split_vs_cc", 3)
    first = device_boundary(*one, 3)
    again = device_boundary(*one, 3, into=first["views"])      # the same call twice into one hist
    assert np.array_equal(again["hist"], 2 * w1["hist"]) and np.array_equal(again["dmax"], w1["dmax"])
    assert np.array_equal(again["a"], w1["a"]) and np.array_equal(again["b"], w1["b"])         # the tables are per call
    a = device_boundary(*one, 3)
    pooled = device_boundary(*two, 3, into=a["views"])         # two different pairs
    assert np.array_equal(pooled["hist"], w1["hist"] + w2["hist"]) and np.array_equal(pooled["dmax"], np.maximum(w1["dmax"], w2["dmax"]))
    assert np.array_equal(pooled["a"], w2["a"])
    assert w1["hist"].sum() > 0 and w2["hist"].sum() > 0 and not np.array_equal(w1["hist"], w2["hist"])


def test_tables_absent_and_a_label_limit_below_the_count():
    A, ka, B, kb = small_pairs()["37x53/cc_vs_shifted"]
    want = host_record("37x53/cc_vs_shifted", 3)
    for tables in ((False, True), (True, False), (False, False)):
        got = device_boundary(A, ka, B, kb, 3, tables=tables)
        assert np.array_equal(got["hist"], want["hist"]) and np.array_equal(got["dmax"], want["dmax"])
        assert (got["a"] is None) == (not tables[0]) and (got["b"] is None) == (not tables[1])
        assert tables[0] is False or np.array_equal(got["a"], want["a"])
        assert tables[1] is False or np.array_equal(got["b"], want["b"])
    zero = device_boundary(A, 0, B, 0, 3)                      # max = 0: every label is background, the tables may be NULL
    assert zero["hist"].sum() == 0 and zero["dmax"].tolist() == [-1, -1] and zero["a"].shape == (3, 0)
    assert ka > 3 and kb > 3
    for la, lb in ((ka - 2, kb), (ka, kb - 3), (1, 2)):
        assert_same(device_boundary(A, la, B, lb, 3), db.boundary_record_numpy(A, la, B, lb, 3), (la, lb))
    assert db.boundary_record_numpy(A, 1, B, 2, 3)["hist"].sum() < want["hist"].sum()


def test_workspace_states():
    """zero / ones / a5, and stale: the bytes a unetdc_split_stats call left at another geometry.  All give the same outputs."""
    from tests.test_gpu_workspace_states import each_state
    from unet_dc_segmentation_amd import _lib
    A, ka, B, kb = small_pairs()["37x53/cc_vs_shifted"]
    want = host_record("37x53/cc_vs_shifted", 64)
    nbytes = _lib.load().unetdc_boundary_distances_workspace(*A.shape)
    seen = []
    for state, ws, _ in each_state(nbytes, "after_split"):
        assert_same(device_boundary(A, ka, B, kb, 64, ws=ws), want, state)
        assert_same(device_boundary(A, ka, B, kb, 64, ws=ws), want, state + ", on its own leftovers")
        seen.append(state)
    assert seen == list(wstates.STATES)


@pytest.mark.parametrize("shape", [(1, 16384), (16384, 1)])
def test_long_sides(shape):
    """The largest LDS row and the largest row count of the grid, a handful of labelled pixels."""
    h, w = shape
    n = h * w
    A, B = np.zeros(n, np.int32), np.zeros(n, np.int32)
    A[[0, 5, 6, 7, 8000, n - 1]] = [1, 2, 2, 2, 3, 4]
    B[[3, 6, 9000, 9001, n - 2]] = [1, 2, 3, 3, 4]
    A, B = A.reshape(h, w), B.reshape(h, w)
    want = db.boundary_record_numpy(A, 4, B, 4, 64)
    assert want["dmax"].tolist() == [1000 * 1000, 1001 * 1001] and want["hist"][:, -1].tolist() == [1, 2]
    assert_same(device_boundary(A, 4, B, 4, 64), want, shape)
    none = np.zeros_like(B)
    assert_same(device_boundary(A, 4, none, 0, 64), db.boundary_record_numpy(A, 4, none, 0, 64), "no finite column")


def test_boundary_batch_on_a_mixed_size_batch(monkeypatch):
    from unet_dc_segmentation_amd.evaluate import boundary_batch, boundary_result
    names = ["37x53/cc_vs_shifted", "7x65/split_vs_cc", "276x408/cc_vs_shifted", "1x1/vs_zeros", "checkerboard"]
    pairs = [small_pairs()[q] for q in names]
    dev = [[torch.from_numpy(np.ascontiguousarray(p[j], dtype=np.int32)).cuda() for p in pairs] for j in (0, 2)]
    kas, kbs = [p[1] for p in pairs], [p[3] for p in pairs]
    calls = {"cpu": 0}
    real_cpu = torch.Tensor.cpu

    def cpu(self, *a, **k):
        calls["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", cpu)
        out = boundary_batch(dev[0], kas, dev[1], kbs, 3)
        assert calls["cpu"] == 1                               # one copy for the whole batch
        for q, rec in zip(names, out):
            assert_same(rec, host_record(q, 3), q)
            assert all(rec[k].dtype == np.int64 for k in KEYS)
        hist = torch.zeros(2, 11, dtype=torch.int64, device="cuda")
        dmax = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        calls["cpu"] = 0
        for _ in range(2):
            pooled = boundary_batch(dev[0], kas, dev[1], kbs, 3, hist=hist, dmax=dmax, objects=False)
        assert calls["cpu"] == 0 and all(r == {"hist": None, "dmax": None, "a": None, "b": None} for r in pooled)
        with_tables = boundary_batch(dev[0], kas, dev[1], kbs, 3, hist=hist, dmax=dmax)
    h, d = boundary_result(hist, dmax)
    assert np.array_equal(h, 3 * sum(host_record(q, 3)["hist"] for q in names))
    assert np.array_equal(d, np.max([host_record(q, 3)["dmax"] for q in names], axis=0)) and d.dtype == np.int64
    for q, rec in zip(names, with_tables):
        assert rec["hist"] is None and np.array_equal(rec["a"], host_record(q, 3)["a"]) and np.array_equal(rec["b"], host_record(q, 3)["b"])
    assert boundary_batch([], [], [], [], 3) == []


def test_match_batch_keeps_the_annotation_labels_on_request():
    from unet_dc_segmentation_amd.evaluate import match_batch
    from tests.test_shape_cpu import cc_labels
    m, g = noise_mask(97, 131, seed=8, sigma=1.5, frac=0.3), noise_mask(97, 131, seed=9, sigma=1.5, frac=0.3)
    lab = cc_labels(m)
    k = int(lab.max())
    dl = torch.from_numpy(lab).cuda()
    areas = np.bincount(lab.ravel(), minlength=k + 1)[1:].astype(np.int64)
    plain = match_batch([dl], [areas], [g])
    kept = match_batch([dl], [areas], [g], keep_labels=True)
    assert "gt_labels" not in plain[0] and sorted(set(kept[0]) - set(plain[0])) == ["gt_labels"]
    assert np.array_equal(kept[0]["gt_labels"].cpu().numpy(), cc_labels(g)) and kept[0]["gt_labels"].dtype == torch.int32
    for q in ("a", "b", "n", "gt_area"):
        assert np.array_equal(plain[0][q], kept[0][q])


def test_cli_device_equals_cpu_path(tmp_path, monkeypatch):
    """quantify_droplets_batch.py --boundary writes the same CSV bytes on the device as on the CPU path, given the same
    probabilities; with --split_touching and --gt_labels there are cuts on both sides."""
    import pandas as pd
    import quantify_droplets_batch as q
    from tests.test_split_cpu import files, run_cli
    assert q.DEVICE == "cuda"
    sizes = ((128, 128), (97, 131), (128, 128))
    masks = [noise_mask(128, 128, seed=70 + i, sigma=2.0, frac=0.4) for i in range(3)]
    masks[2][:] = 0                                            # an image without droplets
    probs = torch.from_numpy(np.stack([probs_of(m) for m in masks]))[:, None]
    base = ["--min_area", "3", "--split_touching"]
    first = run_cli(tmp_path, monkeypatch, "first", base, device="cpu", sizes=sizes, probs=probs)
    lab_dir = tmp_path / "labels"
    lab_dir.mkdir()
    for i in range(3):                                         # the annotation: the run's own label images, moved by a pixel
        from PIL import Image
        lab = np.array(Image.open(first / "predicted_masks" / f"im{i}_labels.png"))
        Image.fromarray(np.roll(lab, 1, axis=1)).save(lab_dir / f"im{i}.png")
    args = base + ["--gt_dir", str(lab_dir), "--gt_labels", "--boundary", "16", "--boundary_tol", "0,1,4"]
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    assert files(dev) == files(cpu) and "boundary_per_image.csv" in files(dev)
    for f in ("all_droplets.csv", "gt_droplets.csv", "boundary_per_image.csv", "match_per_image.csv", "im0_droplets.csv", "im1_droplets.csv"):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    t = pd.read_csv(dev / "boundary_per_image.csv")
    assert t["filename"].tolist() == ["im0.png", "im1.png", "im2.png", "ALL"] and t["bd_px_pred"][0] > 500 and t["bd_px_pred"][2] == 0
    assert 0 < t["nsd_0"][0] < t["nsd_1"][0] <= 1.0 and t["hd"][0] >= 1.0
    assert {"bd_px", "bd_rms", "bd_max"} <= set(pd.read_csv(dev / "all_droplets.csv").columns)


def test_train_device_branch_pools_the_same_integers():
    import train_DC_focal as t
    yp = torch.from_numpy(np.stack([noise_mask(64, 64, seed=80 + i, sigma=2.0, frac=0.4) for i in range(4)])[:, None] > 0)
    yt = torch.from_numpy(np.stack([noise_mask(64, 64, seed=80 + i, sigma=2.2, frac=0.4) for i in range(4)])[:, None] > 0)
    yp[3], yt[2] = False, True                                 # nothing predicted; everything annotated (the frame alone)
    host = t.boundary_report(t.pool_boundary(yp, yt, 8), 8)
    state = t.pool_boundary(yp.cuda(), yt.cuda(), 8)
    assert torch.is_tensor(state[0]) and state[0].is_cuda
    dev = t.boundary_report(state, 8)
    assert np.array_equal(dev["hist"], host["hist"]) and np.array_equal(dev["dmax"], host["dmax"]) and host["hist"].sum() > 500
    assert {k: v for k, v in dev.items() if k not in ("hist", "dmax")} == {k: v for k, v in host.items() if k not in ("hist", "dmax")}
    twice = t.boundary_report(t.pool_boundary(yp.cuda(), yt.cuda(), 8, state), 8)
    assert np.array_equal(twice["hist"], 2 * host["hist"]) and np.array_equal(twice["dmax"], host["dmax"])
