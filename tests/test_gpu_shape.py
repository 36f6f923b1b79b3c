"""GPU: the label map of the plain connected-component path (unetdc_ccl_labels) and the per-droplet shape and intensity
integers (unetdc_label_props, csrc/shape.hip) through the C ABI against scipy and the host path of the same definition
(utils/droplet_shape.py, itself pinned to tests/shape_ref.py on the CPU); then droplets.py and the CLI flag.  Integer
work: bit-exact."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.test_gpu_split import CANARY32, PAD, device_split, plane_result, plane_with_canaries, probs_of, stream, workspace
from tests.test_shape_cpu import INPUTS, cc_labels, gray_plane, split_labels
from tests.test_split_cpu import files, noise_mask, small_masks
from utils import droplet_shape as sh
from utils import droplet_split as ds

pytestmark = pytest.mark.gpu

NQ = len(sh.QUANTITIES)
CANARY64 = -0x0123456789ABCDEF


def device_ccl_labels(mask, min_area=1, max_out=None, ws=None):
    """-> (count, rows [(area, sum_row, sum_col, first_index)], label map); every output between canaries."""
    from unet_dc_segmentation_amd import _lib
    h, w = mask.shape
    lib = _lib.load()
    ws, wptr, nbytes = workspace(lib.unetdc_ccl_labels_workspace(h, w), ws)
    cap = h * w if max_out is None else max_out
    m = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    count = torch.full((1 + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    area = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    root = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    sy = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int64, device="cuda")
    sx = torch.full((cap + 2 * PAD,), CANARY32, dtype=torch.int64, device="cuda")
    lbuf, lab = plane_with_canaries(h, w)
    ptrs = [t[PAD:].data_ptr() for t in (count, area, sy, sx, root)]
    _lib.call("unetdc_ccl_labels", m.data_ptr(), h, w, min_area, wptr, nbytes, *ptrs, lab.data_ptr(), cap, stream())
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
    return n, [tuple(int(x) for x in r) for r in zip(*cols)], plane_result(lbuf, h, w)


def device_props(labels, gray=None, max_out=None, prefill=None):
    """unetdc_label_props -> int64 [NQ][max_out]; the output sits between canary rows that must come back intact.
    prefill: what the output rows hold before the call (a byte value, or an int64 tensor of NQ * max_out stale integers);
    the canary pattern otherwise."""
    from unet_dc_segmentation_amd import _lib
    h, w = labels.shape
    cap = int(labels.max(initial=0)) if max_out is None else max_out
    buf = torch.full((NQ + 2, max(cap, 1)), CANARY64, dtype=torch.int64, device="cuda")
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    g = None if gray is None else torch.from_numpy(np.ascontiguousarray(gray)).cuda()
    flat = buf.view(-1)
    out = flat[max(cap, 1):]
    if isinstance(prefill, int):
        out[:NQ * cap].view(torch.uint8).fill_(prefill)
    elif prefill is not None:
        out[:NQ * cap].copy_(prefill)
    _lib.call("unetdc_label_props", lab.data_ptr(), None if g is None else g.data_ptr(), h, w, out.data_ptr(), cap, stream())
    b = flat.cpu().numpy()
    lo, hi = max(cap, 1), max(cap, 1) + NQ * cap
    assert np.all(b[:lo] == CANARY64) and np.all(b[hi:] == CANARY64), "write outside the output rows"
    return b[lo:hi].reshape(NQ, cap)


def expected_rows(labels, gray, cap):
    """The host path's integers laid out as the device writes them: droplets past cap dropped, numbers without pixels
    (and the grey rows without a grey plane) at their initial values."""
    p = sh.label_props_numpy(labels, gray)
    k = len(p["area"])
    out = np.zeros((NQ, cap), np.int64)
    for j, q in enumerate(sh.QUANTITIES):
        out[j] = sh.MIN_INIT if q.startswith("min_") else sh.MAX_INIT if q.startswith("max_") else 0
        if q in p:
            out[j, :min(k, cap)] = p[q][:cap]
    return out


def assert_props_equal(labels, gray, max_out=None):
    got = device_props(labels, gray, max_out)
    ref = expected_rows(labels, gray, got.shape[1])
    for j, q in enumerate(sh.QUANTITIES):
        assert np.array_equal(got[j], ref[j]), q
    return got


BIG = {"noise9": noise_mask(1040, 1388, seed=9, sigma=6.0, frac=0.35), "noise21": noise_mask(1040, 1388, seed=21, sigma=3.0, frac=0.3)}
SMALL = dict(small_masks())
SMALL.update({f"noise{h}x{w}": noise_mask(h, w, seed=h) for h, w in ((37, 53), (276, 408))})


def scipy_reference(mask, min_area):
    lbl, n = ndimage.label(mask)
    rows = []
    for k, sl in enumerate(ndimage.find_objects(lbl), 1):
        ys, xs = np.nonzero(lbl[sl] == k)
        ys, xs = ys + sl[0].start, xs + sl[1].start
        if len(ys) >= max(min_area, 1):
            rows.append((len(ys), int(ys.sum()), int(xs.sum()), int(ys[0] * mask.shape[1] + xs[0])))
    return cc_labels(mask, min_area), rows


@pytest.mark.parametrize("min_area", [1, 12])
@pytest.mark.parametrize("name", sorted(SMALL) + sorted(BIG))
def test_ccl_labels_equals_scipy_and_ccl_stats(name, min_area):
    m = SMALL[name] if name in SMALL else BIG[name]
    lab, rows = scipy_reference(m, min_area)
    n, drows, dlab = device_ccl_labels(m, min_area)
    assert n == len(rows) and drows == rows
    assert dlab.dtype == np.int32 and np.array_equal(dlab, lab)
    ref = device_split(m, 0, min_area, call="unetdc_ccl_stats")
    assert (n, drows) == ref[:2]


def test_ccl_labels_count_above_max_out():
    m = SMALL["noise276x408"]
    lab, rows = scipy_reference(m, 1)
    assert len(rows) > 40
    n, drows, dlab = device_ccl_labels(m, 1, max_out=17)   # the canary check inside covers entries 17...
    assert n == len(rows) and drows == rows[:17] and np.array_equal(dlab, lab)
    n0, rows0, lab0 = device_ccl_labels(m, 1, max_out=0)
    assert n0 == len(rows) and rows0 == [] and np.array_equal(lab0, lab)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_label_props_equals_host_path_on_small_inputs(name):
    lab = INPUTS[name]
    assert_props_equal(lab, gray_plane(*lab.shape))
    assert_props_equal(lab, None)


def adjacent_label_pairs(lab):
    pairs = set()
    for a, b in ((lab[:, 1:], lab[:, :-1]), (lab[1:], lab[:-1])):
        d = (a != b) & (a > 0) & (b > 0)
        pairs |= {(min(p, q), max(p, q)) for p, q in zip(a[d].tolist(), b[d].tolist())}
    return pairs


@pytest.mark.parametrize("with_gray", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", sorted(BIG))
def test_label_props_equals_host_path_at_full_size(name, split, with_gray):
    m = BIG[name]
    lab = split_labels(m) if split else cc_labels(m)
    # the fixture must exercise the table: many droplets, every edge, single pixels, and touching labels when split
    p = sh.label_props_numpy(lab)
    assert len(p["area"]) >= 100 and (p["area"] == 1).any()
    assert (p["min_y"] == 0).any() and (p["min_x"] == 0).any() and (p["max_y"] == 1039).any() and (p["max_x"] == 1387).any()
    assert not split or len(adjacent_label_pairs(lab)) >= 10
    gray = gray_plane(1040, 1388, seed=3) if with_gray else None
    a = assert_props_equal(lab, gray)
    b = device_props(lab, gray)
    assert np.array_equal(a, b)                              # two runs: bitwise equal


def test_label_props_skips_labels_above_max_out_and_keeps_absent_numbers():
    lab = INPUTS["noise90x120/split"]
    k = int(lab.max())
    assert k > 11
    assert_props_equal(lab, gray_plane(*lab.shape), max_out=11)
    assert_props_equal(lab, None, max_out=k + 9)             # numbers k + 1 .. k + 9 have no pixels
    assert device_props(lab, None, max_out=0).shape == (NQ, 0)


def test_label_props_on_a_device_label_map_of_each_path():
    """The label maps the two device paths write feed the props kernel as they are."""
    m = BIG["noise21"]
    _, _, lab_cc = device_ccl_labels(m, 5)
    _, _, lab_split = device_split(m, 4, 5)
    for lab in (lab_cc, lab_split):
        assert_props_equal(lab, gray_plane(1040, 1388, seed=8))


def host_props(mask, gray, h2):
    lab = cc_labels(mask) if h2 is None else ds.split_labels(mask, h2, 1)[0]
    return lab, sh.label_props_numpy(lab, gray)


def assert_props_dicts_equal(a, b):
    assert sorted(a) == sorted(b)
    for q in a:
        assert np.array_equal(np.asarray(a[q], dtype=np.int64), np.asarray(b[q], dtype=np.int64)), q


@pytest.mark.parametrize("split_depth", [None, 2.0])
def test_batch_with_mixed_sizes_equals_single_images_and_waits_once(monkeypatch, split_depth):
    from unet_dc_segmentation_amd.droplets import mask_and_droplets, mask_and_droplets_batch
    sizes = [(300, 401), (512, 512), (97, 33), (1040, 1388)]
    base = [noise_mask(512, 512, seed=40 + i) for i in range(len(sizes))]
    probs = torch.from_numpy(np.stack([probs_of(m) for m in base])).cuda()
    grays_h = [gray_plane(h, w, seed=70 + i) for i, (h, w) in enumerate(sizes)]
    grays = [torch.from_numpy(g).cuda() for g in grays_h]
    split = {} if split_depth is None else {"split_depth": split_depth}
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
        plain = mask_and_droplets_batch(probs, 0.5, sizes, 1, **split)
        plain_calls = dict(calls)
        calls.update(cpu=0, item=0)
        out = mask_and_droplets_batch(probs, 0.5, sizes, 1, shape=True, gray=grays, return_labels=True, **split)
        # the host waits where it did: on the copy of the counts; then the filled part of the areas and of the sums
        assert calls == plain_calls == {"cpu": 3, "item": 0}
    nogray = mask_and_droplets_batch(probs, 0.5, sizes, 1, shape=True, **split)
    for i, (oh, ow) in enumerate(sizes):
        (mask, a, cy, cx), lab, props = out[i], out[i].labels, out[i].props
        assert plain[i].labels is None and plain[i].props is None and torch.equal(mask, plain[i].mask)
        for x, y in zip(list(plain[i])[1:], (a, cy, cx)):
            assert np.array_equal(x, y)
        one = mask_and_droplets(probs[i], 0.5, (oh, ow), 1, shape=True, gray=grays[i], return_labels=True, **split)
        assert torch.equal(one.mask, mask) and torch.equal(one.labels, lab)
        assert_props_dicts_equal(one.props, props)
        hlab, hp = host_props(mask.cpu().numpy(), grays_h[i], None if split_depth is None else 4)
        assert np.array_equal(lab.cpu().numpy(), hlab)
        assert_props_dicts_equal(props, hp)
        assert nogray[i].labels is None and "Sg" not in nogray[i].props
        assert_props_dicts_equal(nogray[i].props, {q: v for q, v in hp.items() if q not in sh.GRAY_QUANTITIES})


@pytest.mark.parametrize("split_depth", [None, 2.0])
def test_more_droplets_than_the_first_capacity(split_depth):
    from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
    m = np.zeros((2, 64, 64), np.float32)
    m[0, ::2, ::2] = 1.0                                   # 1024 one-pixel droplets, capacity 100
    m[1, 10:20, 10:20] = 1.0
    g = [torch.from_numpy(gray_plane(64, 64, seed=i)).cuda() for i in range(2)]
    split = {} if split_depth is None else {"split_depth": split_depth}
    out = mask_and_droplets_batch(torch.from_numpy(m).cuda(), 0.5, [(64, 64)] * 2, 1, max_droplets=100, shape=True, gray=g, **split)
    for i in range(2):
        hp = host_props((m[i] > 0.5).astype(np.uint8), g[i].cpu().numpy(), None if split_depth is None else 4)[1]
        assert_props_dicts_equal(out[i].props, hp)
    assert len(out[0].area) == 1024 and len(out[1].area) == 1 and out[0].props["P1"].tolist() == [0] * 1024


@pytest.mark.parametrize("extra", [[], ["--split_touching", "--split_depth", "1.5"]])
def test_cli_droplet_shape_device_equals_cpu_path(tmp_path, monkeypatch, extra):
    """quantify_droplets_batch.py --droplet_shape writes the same bytes on the device as on the CPU path, given the same
    512 x 512 probabilities (the network is replaced by fixed maps on both)."""
    import pandas as pd
    import quantify_droplets_batch as q
    from tests.test_split_cpu import run_cli
    assert q.DEVICE == "cuda"
    sizes = ((512, 512), (300, 401), (1040, 1388), (96, 130), (512, 512))
    p = np.stack([np.where(noise_mask(512, 512, seed=60 + i, sigma=4.0, frac=0.4) > 0, 0.9, 0.1) for i in range(len(sizes))])
    p[4] = 0.1
    probs = torch.from_numpy(p.astype(np.float32))[:, None]
    args = ["--droplet_shape", "--min_area", "3", "--px_per_micron", "3.45", "--density_maps"] + extra
    dev = run_cli(tmp_path, monkeypatch, "dev", args, device="cuda", sizes=sizes, probs=probs)
    cpu = run_cli(tmp_path, monkeypatch, "cpu", args, device="cpu", sizes=sizes, probs=probs)
    fd = files(dev)
    assert fd == files(cpu)
    for f in fd:
        if "density" not in f:                             # the density maps have their own device / host comparison
            assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    t = pd.read_csv(dev / "all_droplets.csv")
    assert {"perimeter", "circularity", "touches_border", "intensity_std", "axis_major_micron"} <= set(t.columns) and len(t) > 50
    assert t["touches_border"].any() and not t["touches_border"].all() and (t["circularity"] > 0).any()
