"""GPU: Ripley counts of droplet centroids (unetdc_droplet_points, unetdc_ripley_counts, csrc/spatial.hip) through the C ABI
against the host path of the same definition (utils/spatial_stats.py, itself pinned to the plain loops of tests/spatial_ref.py
on the CPU); then spatial.spatial_stats_batch and the CLI flag.  Integer work: bit-exact.

The shapes are the smallest at which a kernel can go wrong: N around one wave (63, 64, 65) and 1 025 = 4 x 256 + 1 (a fifth pass, of
one point, of the 256 threads that stage the tile; still inside ONE LDS tile of RIPLEY_TILE = 2048 points and one trip of the i loop),
R at both ends and across the 64-bin chunks of the scan (64, 256), widths across a 64-pixel block (130, 401), every kind of
window.  The second and third LDS tile, the later trips of the i loop, a capacity above the point count, tables longer than one
chunk of 256, the other chunk edges of R, the second trip of spatial_sets_kernel and the largest sides are in
tests/test_gpu_grid_caps.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spatial_ref as ref
from tests import workspace_states as wstates
from tests.image_canaries import Canaried
from tests.test_gpu_split import CANARY32, PAD, probs_of, stream
from tests.test_split_cpu import noise_mask
from utils import spatial_stats as ss

pytestmark = pytest.mark.gpu

CANARY64 = -0x35014542_35014542


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).copy()).cuda()


def device_points(area, sy, sx, h, w, window=None, max_points=None):
    """unetdc_droplet_points -> (py, px int64 [N], info [4]); the outputs sit between canaries and only the first N entries may
    have been written; the inputs are unchanged."""
    from unet_dc_segmentation_amd import _lib
    k = len(area)
    assert k >= 1
    cap = k if max_points is None else max_points
    cnt, a, y, x = _dev([k], np.int32), _dev(area, np.int32), _dev(sy, np.int64), _dev(sx, np.int64)
    win = None if window is None else _dev(window, np.uint8)
    outs = [torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda") for _ in range(2)]
    info = torch.full((4 + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    _lib.call("unetdc_droplet_points", cnt.data_ptr(), a.data_ptr(), y.data_ptr(), x.data_ptr(), cap,
              None if win is None else win.data_ptr(), h, w, outs[0][PAD:].data_ptr(), outs[1][PAD:].data_ptr(),
              info[PAD:].data_ptr(), stream())
    i = info.cpu().numpy()
    assert np.all(i[:PAD] == CANARY32) and np.all(i[PAD + 4:] == CANARY32)
    N, flags = int(i[PAD]), int(i[PAD + 3])
    assert 0 <= N <= min(k, cap)
    got = []
    for t in outs:
        v = t.cpu().numpy()
        assert np.all(v[:PAD] == CANARY32) and np.all(v[PAD + cap:] == CANARY32), "write outside a point output"
        if not flags:
            assert np.all(v[PAD + N:] == CANARY32), "write beyond the N points"
        got.append(v[PAD:PAD + N].astype(np.int64))
    assert cnt.item() == k and np.array_equal(a.cpu().numpy(), np.asarray(area, np.int32))
    assert np.array_equal(y.cpu().numpy(), sy) and np.array_equal(x.cpu().numpy(), sx)
    assert window is None or np.array_equal(win.cpu().numpy(), window)
    return got[0], got[1], i[PAD:PAD + 4].astype(np.int64)


def device_counts(py, px, h, w, R, S, seed, window=None, ws=None, max_points=None):
    """unetdc_ripley_counts -> (n, pairs, pairs_all) int64 [(1 + S), R + 1], the workspace view.  The workspace is exactly the
    queried bytes between canaries, the outputs are padded with canaries, the inputs are unchanged."""
    from unet_dc_segmentation_amd import _lib
    N = len(py)
    cap = max(N, 1) if max_points is None else max_points
    lib = _lib.load()
    nbytes = lib.unetdc_ripley_workspace(h, w, cap, R, S)
    assert nbytes > 0
    ws = Canaried(nbytes) if ws is None else ws
    assert ws.nbytes == nbytes
    dy, dx = (torch.cat([_dev(v, np.int32), torch.zeros(cap - N, dtype=torch.int32, device="cuda")]) for v in (py, px))
    npts = _dev([N], np.int32)
    win = None if window is None else _dev(window, np.uint8)
    rows = (1 + S) * (R + 1)
    on = torch.full((rows + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    op, oa = (torch.full((rows + 2 * PAD,), CANARY64, dtype=torch.int64, device="cuda") for _ in range(2))
    _lib.call("unetdc_ripley_counts", dy.data_ptr(), dx.data_ptr(), npts.data_ptr(), cap, None if win is None else win.data_ptr(), h, w,
              R, S, seed, ws.ptr, nbytes, on[PAD:].data_ptr(), op[PAD:].data_ptr(), oa[PAD:].data_ptr(), stream())
    ws.check("workspace")
    got = []
    for t, canary in ((on, CANARY32), (op, CANARY64), (oa, CANARY64)):
        v = t.cpu().numpy()
        assert np.all(v[:PAD] == canary) and np.all(v[PAD + rows:] == canary), "write outside an output"
        got.append(v[PAD:PAD + rows].astype(np.int64).reshape(1 + S, R + 1))
    assert np.array_equal(dy.cpu().numpy()[:N], np.asarray(py, np.int32)) and np.array_equal(dx.cpu().numpy()[:N], np.asarray(px, np.int32))
    assert npts.item() == N and (window is None or np.array_equal(win.cpu().numpy(), window))
    return got[0], got[1], got[2], ws


def assert_counts_equal_host(py, px, h, w, R, S, seed, window=None):
    want = ss.ripley_counts_numpy(py, px, h, w, R, S, seed, window)
    got = device_counts(py, px, h, w, R, S, seed, window)[:3]
    for name, g, v in zip(("n", "pairs", "pairs_all"), got, want):
        assert np.array_equal(g, v), (name, R, S, np.argwhere(g != v)[:5].tolist())
    again = device_counts(py, px, h, w, R, S, seed, window)[:3]                 # two runs: the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    return want


def windows_of(h, w):
    """{kind: window}: NULL, all ones, noisy, with holes, one pixel."""
    rng = np.random.default_rng(h * 1000 + w)
    noisy = (rng.random((h, w)) >= 0.15).astype(np.uint8)
    noisy[h // 2, w // 2] = 1
    holes = np.ones((h, w), np.uint8)
    holes[h // 3:h // 3 + 5, w // 4:w // 4 + 9] = 0
    holes[0, w - 1] = 0 if w > 1 else 1
    if w > 66:
        holes[:, 64:66] = np.where(np.arange(h)[:, None] % 3 == 0, 0, 1)
    holes[h - 1, 0] = 1
    one = np.zeros((h, w), np.uint8)
    one[h - 1, w - 1] = 1                                       # the last pixel of the image
    return {"null": None, "ones": np.ones((h, w), np.uint8), "noisy": noisy, "holes": holes, "one_pixel": one}


@pytest.mark.parametrize("name", sorted(ref.hand_fixtures()))
def test_hand_fixtures(name):
    pts, h, w, R, window, checks = ref.hand_fixtures()[name]
    py, px = [p[0] for p in pts], [p[1] for p in pts]
    n, pairs, pairs_all = assert_counts_equal_host(py, px, h, w, R, 3, 5, window)
    for r, want in checks.get("pairs_all", {}).items():
        assert pairs_all[0][r] == want
    if "e" in checks:
        assert n[0].tolist() == [sum(e >= r for e in checks["e"]) for r in range(R + 1)]
    for other in (1, 64, 256):
        assert_counts_equal_host(py, px, h, w, other, 1, 5, window)


@pytest.mark.parametrize("N", [0, 1, 2, 63, 64, 65, 1025])
def test_point_counts_radii_and_simulations(N):
    h, w = (300, 401) if N > 100 else (96, 130)
    wins = windows_of(h, w)
    for k, (R, S, kind) in enumerate([(1, 0, "null"), (2, 1, "noisy"), (5, 3, "holes"), (64, 1, "null"), (256, 3, "noisy"), (64, 3, "ones")]):
        py, px = ss.simulated_points(100 + N, k, N, h, w, wins[kind])           # inside the window
        want = assert_counts_equal_host(py, px, h, w, R, S, 7 + k, wins[kind])
        assert N < 63 or R < 64 or want[2][0][R] > 0
    if N == 65:                                                # the flow's number of simulations, once
        py, px = ss.simulated_points(1, 0, N, h, w, wins["holes"])
        n, pairs, pairs_all = assert_counts_equal_host(py, px, h, w, 16, 99, 12345, wins["holes"])
        assert len({tuple(r) for r in pairs_all[1:].tolist()}) > 50            # the simulations differ from one another


@pytest.mark.parametrize("hw", [(1, 1), (1, 64), (37, 53), (96, 130), (300, 401)], ids=lambda v: "{}x{}".format(*v))
def test_sizes_and_windows_from_the_droplet_table(hw):
    h, w = hw
    for kind, window in windows_of(h, w).items():
        area, sy, sx, _ = ref.random_case(h, w, 40, "null", seed=h + w)
        want_py, want_px, info = ss.droplet_points(area, sy, sx, h, w, window)
        py, px, got = device_points(area, sy, sx, h, w, window)
        assert np.array_equal(py, want_py) and np.array_equal(px, want_px), kind
        assert got.tolist() == [info["N"], info["n_dropped"], info["A"], 0], kind
        if kind in ("null", "ones"):
            assert info["n_dropped"] == 0
        for R, S in ((5, 3), (64, 1)):
            assert_counts_equal_host(py, px, h, w, R, S, 3, window)
    # a window without a pixel: nothing is kept, A = 0
    py, px, got = device_points(area, sy, sx, h, w, np.zeros((h, w), np.uint8))
    assert len(py) == 0 and got.tolist() == [0, 40, 0, 0]
    assert all(not v.any() for v in device_counts(py, px, h, w, 5, 2, 3, np.zeros((h, w), np.uint8))[:3])


def test_selection_across_a_block_boundary_and_on_the_last_pixel():
    h, w = 6, 130
    win = np.zeros((h, w), np.uint8)
    win[0, 63] = win[0, 64] = win[2, 127] = win[2, 128] = win[h - 1, w - 1] = 1
    py, px = [0] * 40, [63] * 40
    assert_counts_equal_host(py, px, h, w, 64, 3, 3, win)        # the simulated points are the five pixels, 40 draws each
    assert_counts_equal_host(py, px, h, w, 256, 3, 3, win)


def test_every_point_on_one_pixel():
    """N = 1 025 coincident points: every c is 0, every lane of every wave adds to one LDS bin."""
    N, h, w = 1025, 37, 53
    py, px = [20] * N, [30] * N
    n, pairs, pairs_all = assert_counts_equal_host(py, px, h, w, 5, 0, 0)
    assert pairs_all[0].tolist() == [N * (N - 1)] * 6 and n[0].tolist() == [N] * 6 and pairs[0].tolist() == [N * (N - 1)] * 6


def test_a_table_longer_than_max_points_sets_the_flag():
    area, sy, sx, window = ref.random_case(96, 130, 70, "holes", seed=5)
    full = device_points(area, sy, sx, 96, 130, window, max_points=70)
    assert full[2][3] == 0
    short = device_points(area, sy, sx, 96, 130, window, max_points=69)        # the canaries past 69 entries are checked inside
    assert short[2][3] & 1


@pytest.mark.parametrize("state", ["ones", "stale"])
def test_workspace_states(state):
    """The workspace may hold anything on entry: all ones, and what the previous call (another window, radius and seed) left."""
    from unet_dc_segmentation_amd import _lib
    h, w, N, R, S = 96, 130, 65, 64, 3
    wins = windows_of(h, w)
    py, px = ss.simulated_points(9, 0, N, h, w, wins["holes"])
    want = ss.ripley_counts_numpy(py, px, h, w, R, S, 21, wins["holes"])
    ws = Canaried(_lib.load().unetdc_ripley_workspace(h, w, N, R, S))
    if state == "stale":
        qy, qx = ss.simulated_points(10, 0, N, h, w, wins["noisy"])
        device_counts(qy, qx, h, w, R, S, 99, wins["noisy"], ws=ws)
        assert not ws.untouched()
    else:
        wstates.prepare(ws, state)
    for _ in range(2):                                          # and on its own leftovers
        got = device_counts(py, px, h, w, R, S, 21, wins["holes"], ws=ws)[:3]
        assert all(np.array_equal(g, v) for g, v in zip(got, want))
    got = device_counts(py, px, h, w, R, S, 21, None, ws=ws)[:3]                # the window's planes are stale now: not read
    assert all(np.array_equal(g, v) for g, v in zip(got, ss.ripley_counts_numpy(py, px, h, w, R, S, 21)))


def test_refusals_before_any_launch():
    """Host memory stands in for device memory: every refusal comes from host code, before the first launch."""
    from unet_dc_segmentation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    good = dict(h=16, w=16, max_points=8, rmax=4, n_sim=2)
    need = lib.unetdc_ripley_workspace(*good.values())
    assert 0 < need < (1 << 16) - 64

    def counts(ws=a, nbytes=need, py=a, **kw):
        g = dict(good, **kw)
        return lib.unetdc_ripley_counts(py, a, a, g["max_points"], None, g["h"], g["w"], g["rmax"], g["n_sim"], 0, ws, nbytes, a, a, a, None)

    bad = [dict(h=0), dict(w=0), dict(h=16385), dict(w=16385), dict(rmax=0), dict(rmax=257), dict(n_sim=-1), dict(n_sim=1000),
           dict(max_points=0), dict(max_points=(1 << 20) + 1)]
    for kw in bad:
        assert lib.unetdc_ripley_workspace(*dict(good, **kw).values()) == 0, kw
        assert counts(nbytes=1 << 16, **kw) == -1 and b"ripley_counts" in lib.unetdc_last_error(), kw
    assert lib.unetdc_ripley_workspace(16384, 16384, 1 << 20, 256, 999) > 0
    assert counts(py=None) == -1 and b"null" in lib.unetdc_last_error()
    assert counts(ws=None) == -1 and b"null" in lib.unetdc_last_error()
    assert counts(ws=a + 4, nbytes=need) == -1 and b"aligned" in lib.unetdc_last_error()
    assert counts(nbytes=need - 1) == -3 and b"workspace too small" in lib.unetdc_last_error()
    for kw in (dict(h=0), dict(w=16385), dict(max_points=0), dict(max_points=(1 << 20) + 1)):
        g = dict(good, **kw)
        assert lib.unetdc_droplet_points(a, a, a, a, g["max_points"], None, g["h"], g["w"], a, a, a, None) == -1, kw
    assert lib.unetdc_droplet_points(a, a, a, a, 8, None, 16, 16, None, a, a, None) == -1 and b"null" in lib.unetdc_last_error()


def droplet_masks():
    return [noise_mask(120, 160, seed=7, sigma=2.0, frac=0.4), noise_mask(97, 131, seed=8, sigma=1.5, frac=0.3),
            np.zeros((64, 80), np.uint8)]


def test_batch_equals_host_records_and_waits_once(monkeypatch):
    from unet_dc_segmentation_amd import droplets as D
    from unet_dc_segmentation_amd.spatial import spatial_stats_batch
    masks = droplet_masks()
    sizes = [m.shape for m in masks]
    big = max(s[0] for s in sizes), max(s[1] for s in sizes)
    p = np.full((len(masks),) + big, 0.1, np.float32)
    for i, m in enumerate(masks):
        p[i, :m.shape[0], :m.shape[1]] = probs_of(m)
    probs = torch.from_numpy(p).cuda()
    out, sums = D.mask_and_droplets_batch(probs, 0.5, sizes, 2, keep_sums=True, return_labels=True, shape=True)
    assert sums is not None and len(out[0].area) > 8 and len(out[2].area) == 0
    windows = [None, torch.from_numpy(windows_of(*sizes[1])["holes"]).cuda(), None]
    calls = {"cpu": 0}
    real_cpu = torch.Tensor.cpu

    def cpu(self, *a, **k):
        calls["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", cpu)
        recs = spatial_stats_batch(sums, sizes, 16, 3, 77, windows)
    assert calls["cpu"] == 1                                    # exactly one host wait for the batch
    from utils.droplet_match import label_sums
    for d, rec, hw, win in zip(out, recs, sizes, windows):
        want = ss.spatial_record(*label_sums(d.labels.cpu().numpy()), *hw, 16, 3, 77, None if win is None else win.cpu().numpy())
        assert (rec["N"], rec["n_dropped"], rec["A"]) == (want["N"], want["n_dropped"], want["A"])
        for q in ("py", "px", "n", "pairs", "pairs_all"):
            assert rec[q].dtype == np.int64 and np.array_equal(rec[q], want[q]), q
    assert recs[0]["N"] == len(out[0].area) and recs[1]["n_dropped"] > 0 and recs[2]["N"] == 0
    # without the sums the components of the masks are labelled here: the same records at min_area = 1
    out1, sums1 = D.mask_and_droplets_batch(probs, 0.5, sizes, 1, keep_sums=True)
    a = spatial_stats_batch(sums1, sizes, 16, 3, 77, windows)
    b = spatial_stats_batch(None, sizes, 16, 3, 77, windows, masks=[d.mask for d in out1])
    for x, y in zip(a, b):
        assert all(np.array_equal(x[q], y[q]) for q in x)


def test_cli_device_equals_cpu_path(tmp_path, monkeypatch):
    """quantify_droplets_batch.py --spatial_stats writes the same two CSVs on the device as on the CPU path, given the same
    probabilities (the network is replaced by fixed maps on both)."""
    import quantify_droplets_batch as q
    from tests.test_split_cpu import files, run_cli
    assert q.DEVICE == "cuda"
    sizes = ((128, 128), (97, 131))
    masks = [noise_mask(128, 128, seed=60 + i, sigma=2.0, frac=0.4) for i in range(2)]
    probs = torch.from_numpy(np.stack([probs_of(m) for m in masks]))[:, None]
    args = ["--min_area", "3", "--px_per_micron", "3.45", "--spatial_stats", "16", "--spatial_sims", "3"]
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    assert files(dev) == files(cpu)
    for f in ("spatial_stats.csv", "spatial_per_image.csv", "all_droplets.csv", "summary_per_image.csv"):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    import pandas as pd
    assert pd.read_csv(dev / "spatial_per_image.csv")["n_points"].min() > 3
