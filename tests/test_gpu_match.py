"""GPU: the overlap table of two label maps (unetdc_label_overlap, csrc/match.hip) through the C ABI against the host path of
the same definition (utils/droplet_match.py, itself pinned to tests/match_ref.py on the CPU), order included; then
evaluate.py and the CLI flag.  Integer work: bit-exact."""
import numpy as np
import pytest
import torch

from tests import droplet_edge_fixtures as fx
from tests.test_gpu_split import CANARY32, PAD, device_split, probs_of, stream
from tests.test_match_cpu import BIG_PAIRS, areas, big_pair, cc_labels, kmax, shift, small_pairs
from tests.test_split_cpu import files, noise_mask
from utils import droplet_match as dm

pytestmark = pytest.mark.gpu

WS_PAD = 256          # canary bytes on both sides of the workspace
WS_CANARY = 0xA5


def device_overlap_arrays(A, ka, B, kb, max_pairs=None, ws=None):
    """-> (count, int64 arrays (a, b, n) of the first min(count, max_pairs) entries).  The count, the three arrays and the
    workspace sit between canaries; only the first min(count, max_pairs) entries of the arrays may have been written, and on
    overflow nothing past max_pairs.  ws: a prepared Canaried view (tests/image_canaries.py) of exactly the queried bytes to use
    as the workspace, its guards checked here."""
    from unet_dc_segmentation_amd import _lib
    h, w = A.shape
    lib = _lib.load()
    cap = h * w if max_pairs is None else max_pairs
    nbytes = lib.unetdc_label_overlap_workspace(h, w, cap)
    assert nbytes > 0
    if ws is None:
        wbuf = torch.full((nbytes + 2 * WS_PAD,), WS_CANARY, dtype=torch.uint8, device="cuda")
        wptr = wbuf[WS_PAD:].data_ptr()
    else:
        assert ws.nbytes == nbytes
        wbuf, wptr = None, ws.ptr
    la = torch.from_numpy(np.array(A, dtype=np.int32, order="C")).cuda()        # a copy: the fixtures may be read-only
    lb = torch.from_numpy(np.array(B, dtype=np.int32, order="C")).cuda()
    count = torch.full((1 + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    outs = [torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda") for _ in range(3)]
    _lib.call("unetdc_label_overlap", la.data_ptr(), ka, lb.data_ptr(), kb, h, w, wptr, nbytes,
              count[PAD:].data_ptr(), *(t[PAD:].data_ptr() for t in outs), cap, stream())
    c = count.cpu().numpy()
    assert np.all(c[:PAD] == CANARY32) and np.all(c[PAD + 1:] == CANARY32)
    if wbuf is None:
        ws.check("workspace")
    else:
        wsh = wbuf.cpu().numpy()
        assert np.all(wsh[:WS_PAD] == WS_CANARY) and np.all(wsh[WS_PAD + nbytes:] == WS_CANARY), "write outside the workspace"
    n = int(c[PAD])
    assert 0 <= n <= cap + 1
    k = min(n, cap)
    cols = []
    for t in outs:
        v = t.cpu().numpy()
        assert np.all(v[:PAD] == CANARY32) and np.all(v[PAD + k:] == CANARY32), "write outside the first min(count, max_pairs)"
        cols.append(v[PAD:PAD + k].astype(np.int64))
    assert np.array_equal(la.cpu().numpy(), A) and np.array_equal(lb.cpu().numpy(), B)          # the inputs are read only
    return n, tuple(cols)


def device_overlap(A, ka, B, kb, max_pairs=None, ws=None):
    """device_overlap_arrays with the entries as a list of (a, b, n) tuples."""
    n, cols = device_overlap_arrays(A, ka, B, kb, max_pairs, ws)
    return n, list(zip(*(v.tolist() for v in cols)))


def host_table(A, ka, B, kb):
    return list(zip(*(v.tolist() for v in dm.overlap_table_numpy(A, B, ka, kb))))


def assert_equals_host_path(A, ka, B, kb, max_pairs=None):
    ref = host_table(A, ka, B, kb)
    n, got = device_overlap(A, ka, B, kb, max_pairs)
    assert n == len(ref) and got == ref
    return ref


@pytest.mark.parametrize("name", sorted(small_pairs()))
def test_overlap_equals_host_path_on_small_inputs(name):
    A, ka, B, kb = small_pairs()[name]
    ref = assert_equals_host_path(A, ka, B, kb)
    assert_equals_host_path(A, ka, B, kb, max_pairs=len(ref))        # a capacity that just fits


@pytest.mark.parametrize("name", sorted(BIG_PAIRS))
def test_overlap_equals_host_path_at_full_size(name):
    A, ka, B, kb = big_pair(name)
    ref = assert_equals_host_path(A, ka, B, kb, max_pairs=4 * (ka + kb) + 64)
    assert len(ref) == {"noise9_vs_noise21": 1955, "noise9_vs_shifted": 549, "one_vs_noise21": 2537, "one_vs_one": 1}[name]
    if name == "noise9_vs_shifted":
        a, b, n = (np.array(v) for v in zip(*ref))
        image = dm.match_columns(areas(A, ka), areas(B, kb), a, b, n)["image"]
        assert [image[q] for q in dm.TP_NAMES] == [444, 420, 386, 340, 264, 205, 119, 17, 1, 0]
    if name == "one_vs_one":
        assert ref == [(1, 1, 1040 * 1388)]
    assert device_overlap(A, ka, B, kb, max_pairs=4 * (ka + kb) + 64) == (len(ref), ref)         # two runs: bitwise equal


def test_full_size_with_room_for_every_pixel():
    """max_pairs = h * w, the capacity that always suffices: the largest table and the longest sort the call can be asked for."""
    A, ka, B, kb = big_pair("noise9_vs_noise21")
    assert_equals_host_path(A, ka, B, kb)


def test_capacity():
    A, ka, B, kb = small_pairs()["276x408/cc_vs_shifted"]
    ref = host_table(A, ka, B, kb)
    assert len(ref) > 40
    assert_equals_host_path(A, ka, B, kb, max_pairs=len(ref))
    for cap in (len(ref) - 1, 17, 1, 0):                       # the canary check inside covers the entries from cap on
        n, _ = device_overlap(A, ka, B, kb, max_pairs=cap)
        assert n == cap + 1
    z = np.zeros_like(A)
    assert device_overlap(A, ka, z, 0, max_pairs=0) == (0, [])


def assert_arrays_equal_host_path(A, B, max_pairs=None):
    """The long lists: arrays, not tuples.  -> (the host table, the device's arrays)."""
    ka, kb = kmax(A), kmax(B)
    ref = dm.overlap_table_numpy(A, B, ka, kb)
    n, got = device_overlap_arrays(A, ka, B, kb, max_pairs)
    assert n == len(ref[0])
    for q, x, y in zip("abn", got, ref):
        assert np.array_equal(x, y), (q, max_pairs, np.flatnonzero(x != y)[:5])
    return ref, got


@pytest.mark.parametrize("E", [4095, 4096, 4097, 8191, 8192, 8193, 12289])
def test_list_lengths_around_the_sort_chunks(E):
    """Lists of one, two and four LDS chunks of 4096 entries (csrc/pair_table.h): past 4096 the global compare-exchange passes
    and the merge tails of the blocks behind block 0 run.  Tight: the network is the power of two that holds E.  Roomy and
    h * w: the launches of a larger capacity run the list's shorter network, the blocks behind it leave at once.  E - 1:
    overflow, nothing written from the capacity on (the canary check inside device_overlap_arrays)."""
    A, B = fx.pair_count_labels(E)
    want = fx.pair_count_pairs(E)
    ref, _ = assert_arrays_equal_host_path(A, B, max_pairs=E)
    assert len(ref[0]) == E and all(np.array_equal(x, y) for x, y in zip(ref, want))
    assert_arrays_equal_host_path(A, B)                                  # h * w = 24 576: launched for a network of 32 768
    assert_arrays_equal_host_path(A, B, max_pairs=1 << 18)               # outputs of 2^18; the table is cut to h * w
    roomy_A, roomy_B = fx.pair_count_labels(E, (512, 512))               # h * w = 2^18: the capacity is not cut
    roomy, _ = assert_arrays_equal_host_path(roomy_A, roomy_B, max_pairs=1 << 18)
    assert all(np.array_equal(x, y) for x, y in zip(roomy, want))
    n, _ = device_overlap_arrays(A, kmax(A), B, kmax(B), max_pairs=E - 1)
    assert n == E


def test_two_runs_of_a_four_chunk_list_give_equal_bytes():
    A, B = fx.pair_count_labels(12289)
    for cap in (12289, None):
        _, one = assert_arrays_equal_host_path(A, B, max_pairs=cap)
        _, two = assert_arrays_equal_host_path(A, B, max_pairs=cap)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))


def test_label_overlap_recovers_on_a_table_of_more_than_three_chunks():
    """evaluate.label_overlap with 12 289 overlaps: its first capacity 4 (ka + kb) + 64 = 10 140 overflows and the second is
    h * w; from capacity 3 the seventh try has room for 12 288, one short."""
    from unet_dc_segmentation_amd.evaluate import first_capacity, label_overlap
    A, B = fx.pair_count_labels(12289)
    ka, kb = kmax(A), kmax(B)
    assert first_capacity(ka, kb) == 10140 < 12289 and 3 * 4 ** 6 == 12288
    ref = dm.overlap_table_numpy(A, B, ka, kb)
    a_d, b_d = torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(B)).cuda()
    for capacity in (None, 3):
        got = label_overlap(a_d, ka, b_d, kb, capacity=capacity)
        for x, y in zip(got, ref):
            assert x.dtype == np.int64 and np.array_equal(x, y)


def test_labels_out_of_range_are_skipped():
    A, ka, B, kb = small_pairs()["276x408/split_vs_cc"]
    A = A.copy()
    A[0, :9] = -3
    A[5, 5] = -2 ** 31
    assert ka > 8 and kb > 8
    for la, lb in ((ka - 5, kb), (ka, kb - 5), (3, 2), (0, kb), (ka, 0), (ka + 7, kb + 7)):
        ref = assert_equals_host_path(A, la, B, lb)
        assert all(1 <= a <= la and 1 <= b <= lb for a, b, _ in ref)


def test_overlap_of_device_label_maps_of_each_path():
    """The label maps the two device paths write feed the overlap kernel as they are; label_overlap recovers from a first
    capacity that is too small."""
    from unet_dc_segmentation_amd.evaluate import label_overlap
    m = noise_mask(276, 408, seed=7)
    n_split, _, lab_split = device_split(m, 4)
    lab_cc = cc_labels(m)
    ref = dm.overlap_table_numpy(lab_split, lab_cc, n_split, kmax(lab_cc))
    a_d, b_d = torch.from_numpy(lab_split).cuda(), torch.from_numpy(lab_cc).cuda()
    for capacity in (None, 3, 0):
        got = label_overlap(a_d, n_split, b_d, kmax(lab_cc), capacity=capacity)
        for x, y in zip(got, ref):
            assert x.dtype == np.int64 and np.array_equal(x, y)
    assert len(ref[0]) > 3 * 4 ** 2                            # the small capacities take several reruns


def host_match(pred_lab, gt, min_area, gt_are_labels):
    glab = gt if gt_are_labels else dm.gt_labels_numpy(gt, min_area)
    ka = kmax(pred_lab)
    ga, gsy, gsx = dm.label_sums(glab)
    a, b, n = dm.overlap_table_numpy(pred_lab, glab, ka, len(ga))
    return {"a": a, "b": b, "n": n, "gt_area": ga, "gt_sumy": gsy, "gt_sumx": gsx,
            "columns": dm.match_columns(areas(pred_lab, ka), ga, a, b, n)}


def assert_results_equal(x, y):
    for q in ("a", "b", "n", "gt_area", "gt_sumy", "gt_sumx"):
        assert np.array_equal(np.asarray(x[q], dtype=np.int64), np.asarray(y[q], dtype=np.int64)), q
    for side in ("pred", "gt"):
        for q, v in x["columns"][side].items():
            assert np.array_equal(v, y["columns"][side][q]), q
    assert x["columns"]["image"] == y["columns"]["image"]


@pytest.mark.parametrize("gt_are_labels", [False, True])
def test_match_batch_with_mixed_sizes_equals_single_images_and_waits_once(monkeypatch, gt_are_labels):
    from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
    from unet_dc_segmentation_amd.evaluate import match_batch
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
    pred = mask_and_droplets_batch(probs, 0.5, sizes, 3, shape=True, return_labels=True)
    masks = [o.mask.cpu().numpy() for o in pred]
    labs_h = [o.labels.cpu().numpy() for o in pred]
    if gt_are_labels:
        gts = [cc_labels(shift(m, 2, 1)) for m in masks]
    else:
        gts = [shift(m, 2, 1) for m in masks]
        gts[2] = np.zeros(sizes[2], np.uint8)                  # nothing annotated
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", cpu)
        mp.setattr(torch.Tensor, "item", item)
        out = match_batch([o.labels for o in pred], [o.area for o in pred], gts, 5, gt_are_labels)
        # one wait, on the copy of the counts; then the filled part of the int32 and of the int64 outputs: the three copies
        # mask_and_droplets_batch itself makes (tests/test_gpu_shape.py), once more
        assert calls == {"cpu": 3, "item": 0}
    assert len(out) == len(sizes)
    for i in range(len(sizes)):
        assert_results_equal(out[i], host_match(labs_h[i], gts[i], 5, gt_are_labels))
        one = match_batch([pred[i].labels], [pred[i].area], [gts[i]], 5, gt_are_labels)[0]
        assert_results_equal(one, out[i])
    assert out[3]["columns"]["image"]["tp_50"] > 50 and out[3]["columns"]["image"]["n_pred"] > 100


def test_match_batch_recovers_from_small_capacities():
    """More annotated droplets than max_gt, and more pairs than the first capacity of an image: both computed again."""
    from unet_dc_segmentation_amd.evaluate import match_batch
    yy, xx = np.mgrid[0:64, 0:96]
    gt = ((yy % 2 == 0) & (xx % 2 == 0)).astype(np.uint8)      # 1536 one-pixel droplets
    pred = np.ones((64, 96), np.int32)                         # one prediction over all of them: 1536 pairs, first capacity 1096
    out = match_batch([torch.from_numpy(pred).cuda()], [np.array([64 * 96])], [gt], 1, False, max_gt=100)
    assert_results_equal(out[0], host_match(pred, gt, 1, False))
    assert len(out[0]["n"]) == 1536 and out[0]["columns"]["image"]["n_merged"] == 1 and out[0]["columns"]["image"]["n_gt"] == 1536


@pytest.mark.parametrize("extra", [[], ["--split_touching", "--split_depth", "1.5"], ["--droplet_shape"]])
def test_cli_gt_dir_device_equals_cpu_path(tmp_path, monkeypatch, extra):
    """quantify_droplets_batch.py --gt_dir writes the same bytes on the device as on the CPU path, given the same 512 x 512
    probabilities (the network is replaced by fixed maps on both)."""
    import pandas as pd
    from PIL import Image
    import quantify_droplets_batch as q
    from tests.test_split_cpu import run_cli
    assert q.DEVICE == "cuda"
    sizes = ((512, 512), (300, 401), (1040, 1388), (96, 130), (512, 512))
    masks = [noise_mask(512, 512, seed=60 + i, sigma=4.0, frac=0.4) for i in range(len(sizes))]
    p = np.stack([np.where(m > 0, 0.9, 0.1) for m in masks])
    p[4] = 0.1
    probs = torch.from_numpy(p.astype(np.float32))[:, None]
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    for i, (h, w) in enumerate(sizes):                         # image 0: the prediction moved by a pixel; the others: unrelated blobs
        g = shift(masks[0], 1, 1) if i == 0 else noise_mask(h, w, seed=80 + i, sigma=4.0, frac=0.3)
        Image.fromarray(g * 255).save(gt_dir / f"im{i}.png")
    args = ["--min_area", "3", "--px_per_micron", "3.45", "--gt_dir", str(gt_dir), "--gt_min_area", "4"] + extra
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    fd = files(dev)
    assert fd == files(cpu) and {"gt_droplets.csv", "match_per_image.csv"} <= set(fd)
    for f in ("gt_droplets.csv", "match_per_image.csv"):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    whole_tables = "--droplet_shape" in extra or "--split_touching" in extra      # there both paths take centroids from integer sums
    for f in fd:
        if f.endswith("droplets.csv") and f != "gt_droplets.csv":
            if whole_tables:
                assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
            elif (dev / f).stat().st_size > 2:
                a, b = (pd.read_csv(d / f, float_precision="round_trip") for d in (dev, cpu))
                assert list(a.columns) == list(b.columns) and list(a.columns)[-3:] == ["gt_label", "gt_iou", "gt_covered"]
                assert a[["label", "area", "gt_label", "gt_iou", "gt_covered"]].equals(b[["label", "area", "gt_label", "gt_iou", "gt_covered"]])
    t = pd.read_csv(dev / "match_per_image.csv")
    assert t["filename"].tolist() == [f"im{i}.png" for i in range(5)] + ["ALL"]
    assert t["tp_50"][0] > 10 and t["mean_ap"][0] > t["mean_ap"][1] and t["n_pred"][4] == 0 and t["n_gt"][4] > 0
    if "--split_touching" in extra:                            # the run scored against its own label images agrees with itself
        lab_dir = tmp_path / "labels"
        lab_dir.mkdir()
        for i in range(len(sizes)):
            (lab_dir / f"im{i}.png").write_bytes((dev / "predicted_masks" / f"im{i}_labels.png").read_bytes())
        own = ["--min_area", "3", "--gt_dir", str(lab_dir), "--gt_labels"] + extra
        again = run_cli(tmp_path, monkeypatch, "again", own, device="cuda", sizes=sizes, probs=probs)
        t = pd.read_csv(again / "match_per_image.csv")
        assert t["mean_ap"].tolist() == [1.0] * 6 and t["n_pred"].tolist() == t["n_gt"].tolist() and t["n_pred"][5] > 100
