"""GPU: convex hull, solidity and Feret integers per droplet (csrc/hull.hip) through the C ABI against the
plain-loop restatement tests/hull_ref.py, integer for integer, at the smallest sizes where the kernels can go wrong; then
droplets.py and the CLI flag.  Every output and the workspace sit between canaries."""
import numpy as np
import pytest
import torch

from tests import hull_ref
from tests.image_canaries import Canaried, canaried_like
from tests.test_hull_cpu import known_map, random_labels
from tests.workspace_states import STATES, holds, prepare
from utils import droplet_hull as dh

pytestmark = pytest.mark.gpu

Q = dh.QUANTITIES
NH = len(Q)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def rows_needed(lab, max_out):
    """The sum over the labels 1..max_out with pixels of max_y - min_y + 1."""
    total = 0
    for k in np.unique(lab[(lab > 0) & (lab <= max_out)]):
        ys = np.flatnonzero((lab == k).any(axis=1))
        total += int(ys[-1] - ys[0] + 1)
    return total


def device_hull(lab, max_out, max_rows=None, state=None, stale=None, null_out=False, prefill=None):
    """unetdc_label_hull -> (rows int64 [NH, max_out], *out_rows, the workspace view after the call)."""
    from unet_dc_segmentation_amd import _lib
    h, w = lab.shape
    max_rows = rows_needed(lab, max_out) if max_rows is None else max_rows
    need = _lib.load().unetdc_label_hull_workspace(h, w, max_out, max_rows)
    assert need > 0
    src = canaried_like(np.array(lab, dtype=np.int32))
    ws, out, cnt = Canaried(need, align=4), Canaried(NH * max_out * 8, align=8), Canaried(4, align=4)
    if state is not None:
        prepare(ws, state, stale)
    if prefill is not None:
        out.u8.fill_(prefill)
    _lib.call("unetdc_label_hull", src.ptr, max_out, h, w, ws.ptr, need, None if null_out else out.ptr, cnt.ptr, max_rows, _stream())
    torch.cuda.synchronize()
    for v in (src, ws, out, cnt):
        v.check()
    assert np.array_equal(src.numpy(np.int32, h, w), lab)
    return out.numpy(np.int64, NH, max_out), int(cnt.numpy(np.int32, 1)[0]), ws


def assert_equals_ref(rows, ref):
    for j, q in enumerate(Q):
        assert np.array_equal(rows[j], ref[q]), (q, rows[j], ref[q])


def checkerboard(h, w):
    """Single pixels, each its own label of height 1, on every other pixel."""
    lab = np.zeros((h, w), np.int32)
    yy, xx = np.nonzero((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0)
    lab[yy, xx] = np.arange(1, len(yy) + 1)
    return lab


def tall():
    """1040 x 8: label 1 over the full height, a lens whose left and right sides bend by three pixels, notched every fifth row so that
    the chains pop inside every chunk of levels; label 2 a straight column next to it."""
    lab = np.zeros((1040, 8), np.int32)
    for y in range(1040):
        bend = int(round(3 * ((y - 520) / 520) ** 2)) + (y % 5 == 0 and 0 < y < 1039)
        lab[y, bend:7 - bend] = 1
    lab[5:1030, 7] = 2
    return lab


def fixtures():
    out = {"1x1": np.ones((1, 1), np.int32), "1x64": np.ones((1, 64), np.int32)}
    run = np.zeros((1, 65), np.int32)
    run[0, 3:65] = 2                                         # one run across the 64-lane chunk
    out["1x65"] = run
    out["37x53 random"] = random_labels(37, 53, seed=1)
    out["37x53 checkerboard"] = checkerboard(37, 53)
    out["96x130 checkerboard"] = checkerboard(96, 130)       # 6240 labels: past a trip of 4096 of the scan, a partial last tile
    out["96x130 known"] = known_map()[0]
    out["96x130 random"] = random_labels(96, 130, seed=2)
    out["300x401 random"] = random_labels(300, 401, seed=3)
    out["1040x8 tall"] = tall()
    return out


FIXTURES = fixtures()
_refs = {}


def ref_of(name, max_out):
    """The restatement's answer, computed once per (fixture, capacity) and shared."""
    if (name, max_out) not in _refs:
        _refs[name, max_out] = hull_ref.label_hull_ref(FIXTURES[name], max_out)
        for v in _refs[name, max_out].values():
            v.setflags(write=False)
    return _refs[name, max_out]


def capacity(name):
    return 7 if "random" in name else int(FIXTURES[name].max())


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures_equal_the_restatement(name):
    lab, max_out = FIXTURES[name], capacity(name)
    need = rows_needed(lab, max_out)
    rows, n_rows, _ = device_hull(lab, max_out)
    assert n_rows == need
    assert_equals_ref(rows, ref_of(name, max_out))
    again, _, _ = device_hull(lab, max_out, prefill=0xFF)    # two calls, the same bytes, whatever the output held
    assert again.tobytes() == rows.tobytes()
    if name == "96x130 known":
        for k, ints in enumerate(known_map()[1], start=1):
            assert tuple(int(rows[j][k - 1]) for j in range(NH)) == ints, k
    if name == "1040x8 tall":
        assert need == 1040 + 1025 and rows[4][0] >= 8 and rows[4][1] == 4


@pytest.mark.parametrize("max_out", [0, 3, 6, 7, 9, 12])
def test_capacity_below_equal_and_above_the_label_count(max_out):
    """random_labels holds the labels 1..9 without 5: a capacity of 7 skips 8 and 9, one of 12 keeps three numbers without pixels."""
    name = "96x130 random"
    lab = FIXTURES[name]
    rows, n_rows, _ = device_hull(lab, max_out, null_out=max_out == 0)
    assert n_rows == rows_needed(lab, max_out)
    if max_out == 0:
        assert rows.size == 0 and n_rows == 0
        return
    assert_equals_ref(rows, ref_of(name, max_out))
    if max_out >= 5:
        assert not rows[:, 4].any()                          # label 5 has no pixels: the init values
    if max_out == 12:
        assert not rows[:, 9:].any() and rows[4, 8] >= 4


def test_scattered_label_with_empty_rows():
    lab = np.zeros((70, 67), np.int32)
    lab[1, 40] = lab[5, 1] = lab[5, 66] = lab[33, 0] = lab[69, 30] = 1     # 64 rows without a pixel in between
    lab[20:24, 10:14] = 2
    rows, n_rows, _ = device_hull(lab, 2)
    assert n_rows == 69 + 4
    assert_equals_ref(rows, hull_ref.label_hull_ref(lab, 2))


def test_more_chunk_vertices_than_the_lds_pass_holds():
    """hull_chain_kernel merges the 64 chunk chains of a side in LDS when they hold at most 2048 points together, else in memory.
    2111 rows whose leftmost pixel follows a parabola of period 33 (the chunk length at 2112 levels): every level is a vertex of its
    chunk's chain, 2112 points for the second pass.  The right side is one straight column: the LDS pass in the same call."""
    h, w = 2111, 300
    lab = np.zeros((h, w), np.int32)
    r = np.arange(h)
    lab[r, (r % 33 - 16) ** 2] = 1
    lab[r, w - 1] = 1
    xl = (r % 33 - 16) ** 2
    cand = np.minimum(np.append(xl, 10 ** 9), np.append(10 ** 9, xl))                  # the left candidate per corner level
    c = (h + 1 + 63) // 64
    kept = sum(len(dh._chain(list(range(lo, min(lo + c, h + 1))), cand[lo:lo + c].tolist(), 1)) for lo in range(0, h + 1, c))
    assert c == 33 and kept > 2048
    rows, n_rows, _ = device_hull(lab, 1)
    assert n_rows == h
    assert_equals_ref(rows, hull_ref.label_hull_ref(lab, 1))


def test_row_overflow():
    name = "37x53 random"
    lab, ref = FIXTURES[name], ref_of(name, 7)
    need = rows_needed(lab, 7)
    rows, n_rows, _ = device_hull(lab, 7, max_rows=need - 1)          # the canaries around out, the count and the workspace held
    assert n_rows == need
    rows, n_rows, _ = device_hull(lab, 7, max_rows=need)
    assert n_rows == need
    assert_equals_ref(rows, ref)
    rows, n_rows, _ = device_hull(lab, 7, max_rows=0)
    assert n_rows == 1
    rows, n_rows, _ = device_hull(lab, 7, max_rows=37 * 53)
    assert n_rows == need
    assert_equals_ref(rows, ref)


@pytest.mark.parametrize("state", STATES)
def test_workspace_may_hold_anything(state):
    name = "96x130 random"
    lab = FIXTURES[name]
    stale = None
    if state == "stale":                                     # what the stage left at another geometry and capacity
        stale = device_hull(FIXTURES["37x53 checkerboard"], capacity("37x53 checkerboard"))[2].u8.clone()
    rows, n_rows, ws = device_hull(lab, 7, state=state, stale=stale)
    assert n_rows == rows_needed(lab, 7) and not holds(ws, state, stale)
    assert_equals_ref(rows, ref_of(name, 7))
    rows, n_rows, _ = device_hull(lab, 7, max_rows=5, state=state, stale=stale)
    assert n_rows == 6


# ---- droplets.py -------------------------------------------------------------------------------------------------------------------

def batch_inputs():
    from tests.test_split_cpu import noise_mask
    hws = [(120, 160), (97, 131), (64, 80)]
    p = np.stack([np.where(noise_mask(64, 80, seed=70 + i, sigma=2.0, frac=0.35) > 0, 0.8, 0.1).astype(np.float32) for i in range(3)])
    return hws, p


def assert_record_equals_host(d):
    lab = d.labels.cpu().numpy()
    want = dh.label_hull_numpy(lab, len(d.area))
    assert tuple(d.hull) == Q
    for q in Q:
        assert d.hull[q].dtype == np.int64 and np.array_equal(d.hull[q], want[q]), q
    cols, ref = dh.hull_columns(d.hull, d.area), dh.hull_columns(want, np.bincount(lab.ravel(), minlength=len(d.area) + 1)[1:])
    assert list(cols) == list(ref) and all(np.array_equal(cols[k], ref[k]) for k in ref)


@pytest.mark.parametrize("kw", [dict(), dict(shape=True), dict(split_depth=1.0), dict(confidence=0.1), dict(shape=True, confidence=0.1, neighbors=3),
                                dict(split_depth=1.0, shape=True, confidence=0.1)])
def test_through_mask_and_droplets_batch(kw):
    """With and without shape, a split depth and confidence: the hull's rows lie behind theirs in the one int64 allocation."""
    from unet_dc_segmentation_amd import droplets as D
    hws, p = batch_inputs()
    probs = torch.from_numpy(p).cuda()
    before = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, **(kw if kw else dict(shape=True)))
    out = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, hull=True, **kw)
    assert min(len(d.area) for d in out) > 4
    for d, b in zip(out, before):
        assert_record_equals_host(d)
        assert b.hull is None and torch.equal(d.mask, b.mask) and torch.equal(d.labels, b.labels) and np.array_equal(d.area, b.area)
        assert np.array_equal(d.centroid_row, b.centroid_row) and np.array_equal(d.centroid_col, b.centroid_col)
        if "shape" in kw:
            assert all(np.array_equal(d.props[k], b.props[k]) for k in b.props)
        if "confidence" in kw:
            assert all(np.array_equal(d.confidence[k], b.confidence[k]) for k in ("n", "Sq", "Sh", "image"))
    one = D.mask_and_droplets(probs[1], 0.5, hws[1], 2, hull=True, **kw)
    assert one.labels is None and all(np.array_equal(one.hull[q], out[1].hull[q]) for q in Q)


def test_reruns_carry_the_option(monkeypatch):
    from unet_dc_segmentation_amd import droplets as D
    hws, p = batch_inputs()
    probs = torch.from_numpy(p).cuda()
    out = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, hull=True)
    # fewer output slots than droplets: every image is run again with room for all
    again = D.mask_and_droplets_batch(probs, 0.5, hws, 2, max_droplets=4, return_labels=True, hull=True)
    for d, a in zip(out, again):
        assert all(np.array_equal(d.hull[q], a.hull[q]) for q in Q)
    # less row room than the droplets' heights: run again with twice the room until it holds
    names = []
    real = D._lib.call
    with monkeypatch.context() as mp:
        mp.setattr(D, "ROWS_PER_DROPLET", 1)
        mp.setattr(D._lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        small = D.mask_and_droplets_batch(probs, 0.5, hws, 2, max_droplets=16, return_labels=True, hull=True)
    assert names.count("unetdc_label_hull") > 3
    for d, a in zip(out, small):
        assert all(np.array_equal(d.hull[q], a.hull[q]) for q in Q) and torch.equal(d.labels, a.labels)


def test_the_option_adds_no_copy_and_nothing_moves_without_it(monkeypatch):
    from unet_dc_segmentation_amd import droplets as D
    hws, p = batch_inputs()
    probs = torch.from_numpy(p).cuda()
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
        plain = D.mask_and_droplets_batch(probs, 0.5, hws, 2)
        off = list(calls["names"])
        assert calls["cpu"] == 3 and "unetdc_label_hull" not in off and "unetdc_ccl_stats" in off
        explicit = D.mask_and_droplets_batch(probs, 0.5, hws, 2, hull=False)
        assert calls["names"] == off + off
        calls.update(cpu=0, names=[])
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, shape=True)
        shape_off = list(calls["names"])
        calls.update(cpu=0, names=[])
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, shape=True, hull=True)
        assert calls["cpu"] == 3
        assert [n for n in calls["names"] if n != "unetdc_label_hull"] == shape_off and calls["names"].count("unetdc_label_hull") == 3
    for a, b in zip(plain, explicit):
        assert torch.equal(a.mask, b.mask) and a.area.tobytes() == b.area.tobytes() and a.centroid_row.tobytes() == b.centroid_row.tobytes()
        assert a.centroid_col.tobytes() == b.centroid_col.tobytes() and a.hull is None and b.hull is None and a.labels is None


# ---- the script ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,args,sizes", [
    ("plain", ["--droplet_hull"], ((96, 96), (80, 112), (64, 64))),
    ("combo", ["--droplet_hull", "0.95", "--split_touching", "--droplet_shape", "--neighbors", "3", "--confidence", "--tta", "2",
               "--px_per_micron", "2"], ((96, 96), (80, 112), (64, 64))),
    ("tiled", ["--droplet_hull", "--tile", "64", "--tile_overlap", "16"], ((96, 130),))])
def test_cli_device_equals_cpu_path(tmp_path, monkeypatch, tag, args, sizes):
    """quantify_droplets_batch.py --droplet_hull on the device against its CPU path on the synthetic set: the network is the exact
    stand-in of tests/test_tta_cpu.py, so the label maps and with them every integer agree; the float columns are the same
    float64 formulas on equal integers: identical bytes."""
    import pandas as pd
    import quantify_droplets_batch as q
    from tests.test_confidence_cpu import files, run_script
    assert q.DEVICE == "cuda"
    dev = run_script(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes)
    cpu = run_script(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes)
    assert files(dev) == files(cpu)
    for f in files(dev):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    t = pd.read_csv(dev / "all_droplets.csv")
    assert len(t) > 3 and set(dh.COLUMN_NAMES) <= set(t.columns) and t["solidity"].between(0, 1).all()
    assert set(dh.SUMMARY_NAMES) <= set(pd.read_csv(dev / "summary_per_image.csv").columns)
