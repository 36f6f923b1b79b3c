"""GPU: droplet neighbourhoods (unetdc_label_neighbors, csrc/neighbors.hip) through the C ABI against the host path of the
same definition (utils/droplet_neighbors.py, itself pinned to the brute force of tests/neighbors_ref.py on the CPU), order
included; then droplets.py and the CLI flag.  Integer work: bit-exact."""
import numpy as np
import pytest
import torch

from tests import neighbors_ref as ref
from tests import workspace_states as wstates
from tests.image_canaries import Canaried
from tests.test_gpu_split import CANARY32, PAD, probs_of, stream
from tests.test_split_cpu import noise_mask
from utils import droplet_neighbors as dn

pytestmark = pytest.mark.gpu

RADII = (1, 2, 5, 32, 64)


def device_neighbors_arrays(lab, k, G, max_pairs=None, ws=None):
    """-> (count, int64 arrays (a, b, d2) of the first min(count, max_pairs) entries, {column: int64 [k]}, the workspace view).
    The count, the three pair arrays, the five per-label arrays and the workspace sit between canaries; only the first
    min(count, max_pairs) entries of the pair arrays may have been written.  ws: a prepared Canaried view of exactly the
    queried bytes to use as the workspace."""
    from unet_dc_segmentation_amd import _lib
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    h, w = lab.shape
    lib = _lib.load()
    cap = k * (k - 1) // 2 if max_pairs is None else max_pairs
    nbytes = lib.unetdc_label_neighbors_workspace(h, w, k, cap)
    assert nbytes > 0
    if ws is None:
        ws = Canaried(nbytes)
    assert ws.nbytes == nbytes
    dl = torch.from_numpy(lab.copy()).cuda()
    count = torch.full((1 + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    pairs = [torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda") for _ in range(3)]
    cols = [torch.full((k + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda") for _ in range(5)]
    _lib.call("unetdc_label_neighbors", dl.data_ptr(), k, h, w, G, ws.ptr, nbytes, count[PAD:].data_ptr(),
              *((t[PAD:].data_ptr() if cap else None) for t in pairs), cap, *((t[PAD:].data_ptr() if k else None) for t in cols), stream())
    c = count.cpu().numpy()
    assert np.all(c[:PAD] == CANARY32) and np.all(c[PAD + 1:] == CANARY32)
    ws.check("workspace")
    n = int(c[PAD])
    assert 0 <= n <= cap + 1
    m = min(n, cap)
    got = []
    for t in pairs:
        v = t.cpu().numpy()
        assert np.all(v[:PAD] == CANARY32) and np.all(v[PAD + m:] == CANARY32), "write outside the first min(count, max_pairs)"
        got.append(v[PAD:PAD + m].astype(np.int64))
    out = {}
    for q, t in zip(dn.COLUMN_NAMES, cols):
        v = t.cpu().numpy()
        assert np.all(v[:PAD] == CANARY32) and np.all(v[PAD + k:] == CANARY32), "write outside a per-label output"
        out[q] = v[PAD:PAD + k].astype(np.int64)
    assert np.array_equal(dl.cpu().numpy(), lab)               # the input is read only
    return n, tuple(got), out, ws


def device_neighbors(lab, k, G, max_pairs=None, ws=None):
    """device_neighbors_arrays with the pairs as a list of (a, b, d2) tuples and the columns as lists."""
    n, got, out, ws = device_neighbors_arrays(lab, k, G, max_pairs, ws)
    return n, list(zip(*(v.tolist() for v in got))), {q: v.tolist() for q, v in out.items()}, ws


def host_record(lab, k, G):
    rec = dn.neighbors_numpy(lab, k, G)
    return list(zip(*(rec["pairs"][q].tolist() for q in ("a", "b", "d2")))), {q: rec[q].tolist() for q in dn.COLUMN_NAMES}


def assert_equals_host_path(lab, k, G, max_pairs=None):
    pairs, cols = host_record(lab, k, G)
    n, got, gcols, _ = device_neighbors(lab, k, G, max_pairs)
    assert n == len(pairs) and got == pairs, (G, got[:5], pairs[:5])
    assert gcols == cols, G
    n2, got2, gcols2, _ = device_neighbors(lab, k, G, max_pairs)            # two runs: bitwise equal, pair order included
    assert (n2, got2, gcols2) == (n, got, gcols)
    return pairs


@pytest.mark.parametrize("name", sorted(ref.hand_fixtures()))
def test_hand_fixtures(name):
    lab, k, G, want = ref.hand_fixtures()[name]
    assert assert_equals_host_path(lab, k, G) == want
    assert_equals_host_path(lab, k, G, max_pairs=len(want))    # a capacity that just fits, 0 included
    for other in RADII:
        assert_equals_host_path(lab, k, other)


@pytest.mark.parametrize("name", sorted(ref.edge_maps()))
def test_edge_geometries(name):
    lab, k = ref.edge_maps()[name]
    for G in RADII:
        pairs = assert_equals_host_path(lab, k, G)
        assert all(1 <= a < b <= k for a, b, _ in pairs)


@pytest.mark.parametrize("G", RADII)
def test_random_maps(G):
    lab, n = ref.random_map()
    pairs = assert_equals_host_path(lab, n, G)
    assert G < 5 or len(pairs) > n // 2
    assert_equals_host_path(lab, n // 2, G)                    # half the labels are background
    tlab, tk = ref.touching_map()
    assert_equals_host_path(tlab, tk, G)


def seam_maps():
    """Pairs that straddle the kernels' own boundaries: the 16 x 64 tiles of the border list (x = 63|64, 127|128, widths 65 and
    129; rows 15|16, 31|32, heights 17 and 33) and the 64-column trips of the scan, which start at x - G; a droplet in the last
    column and row whose disc hangs over the image on all four sides."""
    out = {}
    for w in (65, 129, 131):
        m = np.zeros((5, w), np.int32)
        m[2, 63], m[2, 64] = 1, 2                              # 4-adjacent across the unit seam
        m[0, 62], m[4, 65 if w > 65 else 64] = 3, 4
        if w > 128:
            m[1, 127], m[3, 128] = 5, 6                        # diagonal across the second seam
            m[4, w - 1] = 7
        out[f"seams_w{w}"] = (m, int(m.max()))
    for h in (17, 33):                                         # the 16-row tiles of the border list: rows 15|16 and 31|32
        m = np.zeros((h, 70), np.int32)
        m[15, 5], m[16, 5] = 1, 2                              # 4-adjacent across the tile seam
        m[14:17, 63:66] = 3                                    # a droplet over the corner of four tiles
        m[0, 69], m[h - 1, 0], m[h - 1, 69] = 4, 5, 6
        if h > 32:
            m[31, 30], m[32, 31] = 7, 8                        # diagonal across the second seam
        out[f"row_tiles_h{h}"] = (m, int(m.max()))
    small = np.zeros((7, 9), np.int32)
    small[6, 8], small[0, 0], small[0, 8], small[6, 0], small[3, 4] = 1, 2, 3, 4, 5
    out["window_over_every_edge"] = (small, 5)
    far = np.zeros((3, 200), np.int32)
    far[1, 0], far[1, 64], far[1, 128], far[1, 192], far[0, 199] = 1, 2, 3, 4, 5     # partners exactly 64 columns away
    out["partners_64_columns_apart"] = (far, 5)
    tall = np.zeros((200, 3), np.int32)
    tall[0, 1], tall[64, 1], tall[128, 1], tall[199, 2] = 1, 2, 3, 4
    out["partners_64_rows_apart"] = (tall, 4)
    return out


@pytest.mark.parametrize("name", sorted(seam_maps()))
def test_kernel_seams(name):
    lab, k = seam_maps()[name]
    for G in RADII + (63,):
        assert_equals_host_path(lab, k, G)
    if name.startswith("partners"):
        assert [d for _, _, d in host_record(lab, k, 64)[0]].count(4096) >= 2 and host_record(lab, k, 63)[0] != host_record(lab, k, 64)[0]


def test_hub_and_bars():
    """One 1 x 280 bar with 90 single pixels two rows below it: degree 90, every insert contends on one label.  Two 1 x 280 bars
    three rows apart: thousands of hits, one pair."""
    hub = np.zeros((4, 280), np.int32)
    hub[0, :] = 1
    hub[2, 0:270:3] = np.arange(2, 92)
    pairs = assert_equals_host_path(hub, 91, 2)
    assert len(pairs) == 90 and all(a == 1 and d == 4 for a, _, d in pairs)
    assert device_neighbors(hub, 91, 2)[2]["degree"][0] == 90
    assert len(assert_equals_host_path(hub, 91, 5)) > 90
    bars = np.zeros((6, 280), np.int32)
    bars[1, :], bars[4, :] = 1, 2
    for G in (2, 3, 5, 64):
        assert assert_equals_host_path(bars, 2, G) == ([(1, 2, 9)] if G >= 3 else [])


def test_more_border_pixels_than_the_scan_grid():
    """200 x 300 in 2 x 2 cells of 39 labels: nearly every pixel is a border pixel, several trips of the scan's capped grid."""
    lab, k = ref.touching_map(200, 300, 8, 2)
    pairs = assert_equals_host_path(lab, k, 2)
    assert len(pairs) == k * (k - 1) // 2


def test_capacity():
    lab, n = ref.random_map()
    pairs, cols = host_record(lab, n, 5)
    assert len(pairs) > 40
    assert_equals_host_path(lab, n, 5, max_pairs=len(pairs))
    for cap in (len(pairs) - 1, 17, 1, 0):                     # the canary check inside covers the entries from cap on
        assert device_neighbors(lab, n, 5, max_pairs=cap)[0] == cap + 1
    assert device_neighbors(np.zeros_like(lab), n, 5, max_pairs=0)[:2] == (0, [])
    assert device_neighbors(lab, 0, 5, max_pairs=0)[:3] == (0, [], {q: [] for q in dn.COLUMN_NAMES})


def assert_arrays_equal_reference(lab, k, G, max_pairs, pairs=None):
    """The long lists: the device's arrays against offset_pairs (tests/neighbors_ref.py, pinned to the host path on the CPU)
    and the host columns of that list, twice: two runs give equal bytes, pair order included.  -> the device's record."""
    pairs = ref.offset_pairs(lab, k, G) if pairs is None else pairs
    cols = dn.neighbor_columns(pairs, k, dn.present_labels(lab, k))
    runs = [device_neighbors_arrays(lab, k, G, max_pairs)[:3] for _ in range(2)]
    n, got, gcols = runs[0]
    assert n == len(pairs[0])
    for q, x, y in zip(("a", "b", "d2"), got, pairs):
        assert np.array_equal(x, y), (q, G, max_pairs, np.flatnonzero(x != y)[:5])
    for q in dn.COLUMN_NAMES:
        assert np.array_equal(gcols[q], cols[q]), (q, G, max_pairs, np.flatnonzero(gcols[q] != cols[q])[:5])
    assert runs[1][0] == n and all(x.tobytes() == y.tobytes() for x, y in zip(got, runs[1][1]))
    assert all(gcols[q].tobytes() == runs[1][2][q].tobytes() for q in dn.COLUMN_NAMES)
    return n, got, gcols


@pytest.mark.parametrize("lattice", ref.LATTICES, ids=lambda v: "{}x{}_step{}_G{}".format(*v[:4]))
def test_lattices_of_more_pairs_than_a_sort_chunk(lattice):
    """Two, four and sixteen LDS chunks of pairs (csrc/pair_table.h) in this file's copy of the sort: the global passes, the
    merge tails behind block 0, and thousands of labels for the union and the 64-bit minimum, whose ties the smaller label
    wins.  max_pairs is always given: the helper's default k (k - 1) / 2 would be a table of gigabytes."""
    h, w, step, G, k, n = lattice
    lab, _ = ref.lattice_map(h, w, step)
    pairs = ref.offset_pairs(lab, k, G)
    assert len(pairs[0]) == n > 4096
    assert_arrays_equal_reference(lab, k, G, n, pairs)                   # exact
    _, _, cols = assert_arrays_equal_reference(lab, k, G, 1 << 16, pairs)
    assert (cols["cluster"] == 1).all() and (cols["cluster_size"] == k).all() and (cols["nn_d2"] == step * step).all()
    assert device_neighbors_arrays(lab, k, G, n - 1)[0] == n             # overflow: the canaries from n - 1 on are checked inside
    half = ref.offset_pairs(lab, k // 2, G)                              # half the labels are background
    assert 0 < len(half[0]) < n // 2
    assert_arrays_equal_reference(lab, k // 2, G, len(half[0]), half)
    assert_arrays_equal_reference(lab, k // 2, G, 1 << 16, half)


def test_patches_of_known_cluster_sizes():
    """Thousands of clusters of one to nine droplets and a few labels without a pixel, over three sort chunks of pairs."""
    lab, K, cluster, size = ref.patch_map()
    for cap in (1 << 14, 1 << 16):
        n, _, cols = assert_arrays_equal_reference(lab, K, ref.PATCH_G, cap)
        assert 3 * 4096 < n <= 1 << 14
        assert np.array_equal(cols["cluster"], cluster) and np.array_equal(cols["cluster_size"], size)


def test_batch_at_the_production_pair_room():
    """260 x 260 with a droplet every second pixel: 16 900 droplets and 33 540 pairs, more than PAIR_ROOM = 2^14.  The first launch
    overflows at the capacity production uses, the retries double it."""
    from unet_dc_segmentation_amd import droplets as D
    m = np.zeros((260, 260), np.uint8)
    m[::2, ::2] = 1
    probs = torch.from_numpy(probs_of(m)[None]).cuda()
    assert D.PAIR_ROOM == 1 << 14 and 2 * D.PAIR_ROOM < 33540
    out = D.mask_and_droplets_batch(probs, 0.5, [m.shape], 1, max_droplets=1 << 15, return_labels=True, neighbors=2)[0]
    assert len(out.area) == 16900 and (out.area == 1).all()
    assert assert_record_equals_host(out, 2) == 33540
    lab = out.labels.cpu().numpy()
    assert all(np.array_equal(out.neighbors["pairs"][q], v) for q, v in zip(("a", "b", "d2"), ref.offset_pairs(lab, 16900, 2)))


@pytest.mark.parametrize("state", ["ones", "stale"])
def test_workspace_states(state):
    """The workspace may hold anything on entry: all ones, and what the previous call (another map, another radius) left."""
    from unet_dc_segmentation_amd import _lib
    lab, n = ref.random_map()
    want = device_neighbors(lab, n, 5)[:3]
    nbytes = _lib.load().unetdc_label_neighbors_workspace(*lab.shape, n, n * (n - 1) // 2)
    ws = Canaried(nbytes)
    if state == "stale":
        tlab, _ = ref.touching_map(*lab.shape, 3, 5)
        device_neighbors(tlab, n, 32, ws=ws)
        assert not ws.untouched()
    else:
        wstates.prepare(ws, state)
    assert device_neighbors(lab, n, 5, ws=ws)[:3] == want
    assert device_neighbors(lab, n, 5, ws=ws)[:3] == want      # and on its own leftovers


def droplet_masks():
    return [noise_mask(120, 160, seed=7, sigma=2.0, frac=0.4), noise_mask(97, 131, seed=8, sigma=1.5, frac=0.3),
            np.zeros((64, 80), np.uint8)]


def assert_record_equals_host(d, G):
    lab = d.labels.cpu().numpy()
    want = dn.neighbors_numpy(lab, len(d.area), G)
    for q in ("a", "b", "d2"):
        assert d.neighbors["pairs"][q].dtype == np.int64 and np.array_equal(d.neighbors["pairs"][q], want["pairs"][q]), q
    for q in dn.COLUMN_NAMES:
        assert d.neighbors[q].dtype == np.int64 and np.array_equal(d.neighbors[q], want[q]), q
    return len(want["pairs"]["a"])


@pytest.mark.parametrize("kw", [dict(min_area=1), dict(min_area=4), dict(min_area=1, split_depth=1.0), dict(min_area=1, shape=True),
                                dict(min_area=1, max_hole_area=-1, thresh_low=0.2)])
def test_through_mask_and_droplets_batch(monkeypatch, kw):
    from unet_dc_segmentation_amd import droplets as D
    masks = droplet_masks()
    sizes = [m.shape for m in masks]
    big = max(s[0] for s in sizes), max(s[1] for s in sizes)
    p = np.full((len(masks),) + big, 0.1, np.float32)
    out_hws = [big] * len(masks)
    for i, m in enumerate(masks):
        p[i, :m.shape[0], :m.shape[1]] = probs_of(m)
    probs = torch.from_numpy(p).cuda()
    min_area = kw.pop("min_area")
    G = 3
    before_kw = kw if "split_depth" in kw else dict(kw, shape=True)        # without a split depth the label map came from the shape route
    before = D.mask_and_droplets_batch(probs, 0.5, out_hws, min_area, return_labels=True, **before_kw)
    out = D.mask_and_droplets_batch(probs, 0.5, out_hws, min_area, return_labels=True, neighbors=G, **kw)
    n_pairs = [assert_record_equals_host(d, G) for d in out]
    assert n_pairs[0] > 8 and n_pairs[2] == 0
    for d, b in zip(out, before):                              # the other fields are those of a call without the option
        assert b.neighbors is None and torch.equal(d.mask, b.mask) and torch.equal(d.labels, b.labels)
        assert np.array_equal(d.area, b.area) and np.array_equal(d.centroid_row, b.centroid_row)
        assert np.array_equal(d.centroid_col, b.centroid_col) and np.array_equal(d.clean_counts, b.clean_counts)
    # a pair capacity forced small takes the retry and gives the same record
    monkeypatch.setattr(D, "PAIR_ROOM", 2)
    again = D.mask_and_droplets_batch(probs, 0.5, out_hws, min_area, return_labels=True, neighbors=G, **kw)
    for d, a in zip(out, again):
        for q in ("a", "b", "d2"):
            assert np.array_equal(d.neighbors["pairs"][q], a.neighbors["pairs"][q])
        for q in dn.COLUMN_NAMES:
            assert np.array_equal(d.neighbors[q], a.neighbors[q])
    one = D.mask_and_droplets(probs[0], 0.5, big, min_area, neighbors=G, **kw)
    assert one.labels is None and np.array_equal(one.neighbors["pairs"]["d2"], out[0].neighbors["pairs"]["d2"])


def test_option_off_adds_no_copy_and_option_on_two(monkeypatch):
    from unet_dc_segmentation_amd import droplets as D
    m = droplet_masks()[0]
    probs = torch.from_numpy(probs_of(m)[None]).cuda()
    calls = {"cpu": 0}
    real_cpu = torch.Tensor.cpu

    def cpu(self, *a, **k):
        calls["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", cpu)
        off = D.mask_and_droplets_batch(probs, 0.5, [m.shape], 1)
        assert calls["cpu"] == 3 and off[0].neighbors is None
        D.mask_and_droplets_batch(probs, 0.5, [m.shape], 1, neighbors=5)
        assert calls["cpu"] == 3 + 5


def test_cli_device_equals_cpu_path(tmp_path, monkeypatch):
    """quantify_droplets_batch.py --neighbors writes the same three CSVs on the device as on the CPU path, given the same
    probabilities (the network is replaced by fixed maps on both)."""
    import quantify_droplets_batch as q
    from tests.test_split_cpu import files, run_cli
    assert q.DEVICE == "cuda"
    sizes = ((128, 128), (97, 131))
    masks = [noise_mask(128, 128, seed=60 + i, sigma=2.0, frac=0.4) for i in range(2)]
    probs = torch.from_numpy(np.stack([probs_of(m) for m in masks]))[:, None]
    args = ["--min_area", "3", "--px_per_micron", "3.45", "--neighbors", "4"]
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    assert files(dev) == files(cpu)
    for f in ("all_droplets.csv", "droplet_contacts.csv", "summary_per_image.csv", "im0_droplets.csv", "im1_droplets.csv"):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    import pandas as pd
    assert pd.read_csv(dev / "summary_per_image.csv")["n_contacts"].min() > 3
