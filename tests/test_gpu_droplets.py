"""GPU: droplet quantification kernels (csrc/ccl.hip) against the SciPy restatement of the reference's quantify()
(/root/reference/quantify_droplets_batch.py:81-95): exact areas, centroids, label order; cv2's nearest-neighbour index
rule; the strict `>` threshold.  Integer / byte work: the bar is bit-exact."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import image_edge_fixtures as fx
from tests.image_canaries import Canaried

pytestmark = pytest.mark.gpu


def _reference_table(mask, min_area):
    import quantify_droplets_batch as q
    return q.quantify(mask.astype(np.uint8), min_area, 3.45)


def _device_table(probs, thresh, out_hw, min_area):
    import quantify_droplets_batch as q
    return q.quantify_device(torch.from_numpy(probs).cuda(), thresh, out_hw, min_area, 3.45)


def _spiral(n):
    """One long thin 4-connected spiral: the worst case for label propagation (a root thousands of hops away)."""
    m = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    lo_y, hi_y, lo_x, hi_x = 0, n - 1, 0, n - 1
    while lo_y <= hi_y and lo_x <= hi_x:
        m[y, x] = 1
        ny, nx = y + dy, x + dx
        if not (lo_y <= ny <= hi_y and lo_x <= nx <= hi_x):
            if (dy, dx) == (0, 1):
                lo_y += 2
            elif (dy, dx) == (1, 0):
                hi_x -= 2
            elif (dy, dx) == (0, -1):
                hi_y -= 2
            else:
                lo_x += 2
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            if not (lo_y - 2 <= ny <= hi_y + 2 and lo_x - 2 <= nx <= hi_x + 2) or m[min(max(ny, 0), n - 1), min(max(nx, 0), n - 1)]:
                break
        y, x = ny, nx
        if not (0 <= y < n and 0 <= x < n):
            break
    return m


@pytest.mark.parametrize("case", ["random", "discs", "spiral", "empty", "full", "checker"])
@pytest.mark.parametrize("min_area", [1, 5])
def test_ccl_table_matches_scipy(case, min_area):
    rng = np.random.default_rng(7)
    h, w = 384, 520
    if case == "random":
        m = (rng.random((h, w)) < 0.55).astype(np.uint8)         # near the percolation threshold: huge ragged components
    elif case == "discs":
        m = np.zeros((h, w), np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        for _ in range(300):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, 14)
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    elif case == "spiral":
        m = np.zeros((h, w), np.uint8)
        m[:384, :384] = _spiral(384)
        m[10, 500] = 1                                        # plus a one-pixel object
    elif case == "empty":
        m = np.zeros((h, w), np.uint8)
    elif case == "full":
        m = np.ones((h, w), np.uint8)
    else:
        m = ((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0).astype(np.uint8)   # 4-connectivity: every pixel its own object
    probs = np.where(m > 0, 0.9, 0.1).astype(np.float32)
    mask, df = _device_table(probs, 0.3, (h, w), min_area)
    assert mask.dtype == np.uint8 and np.array_equal(mask, m)
    ref = _reference_table(m, min_area)
    assert len(df) == len(ref)
    if len(ref):
        assert list(df.columns) == list(ref.columns)
        assert np.array_equal(df["label"].to_numpy(), ref["label"].to_numpy())
        assert np.array_equal(df["area"].to_numpy(), ref["area"].to_numpy())
        np.testing.assert_allclose(df["centroid-0"].to_numpy(), ref["centroid-0"].to_numpy(), rtol=0, atol=1e-9)
        np.testing.assert_allclose(df["centroid-1"].to_numpy(), ref["centroid-1"].to_numpy(), rtol=0, atol=1e-9)
        np.testing.assert_allclose(df["equivalent_diameter"].to_numpy(), ref["equivalent_diameter"].to_numpy(), rtol=1e-15)


@pytest.mark.parametrize("mode", ["nearest", "reference"])
@pytest.mark.parametrize("out_hw", [(512, 512), (276, 408), (1037, 1388), (97, 33)])
def test_threshold_is_strict_and_resize_follows_cv2_rule(out_hw, mode, monkeypatch):
    """nearest: mask = cv2.resize((p > thresh).astype(uint8), (ow, oh), interpolation=INTER_NEAREST): strict compare on the
    fp32 value (a probability exactly at the threshold is background), source index min(floor(d * src / dst), src - 1).
    reference (the default): what the reference's positional-flag call computes, OpenCV's 8-bit INTER_LINEAR on the {0,1}
    mask (utils/data_loader.py:resize_linear_cv2_u8 restates it; both rules unpinned against cv2, which is not installed)."""
    from unet_dc_segmentation_amd import droplets
    from unet_dc_segmentation_amd.droplets import mask_and_droplets, resize_mask_like_reference
    monkeypatch.setattr(droplets, "MASK_RESIZE", mode)
    resize_nearest_cv2 = resize_mask_like_reference
    g = torch.Generator().manual_seed(5)
    p = torch.rand(512, 512, generator=g)
    thresh = float(np.float32(0.3))
    p[::7, ::5] = thresh                                       # exactly at the threshold
    p[3::11, 2::13] = float(np.nextafter(np.float32(0.3), np.float32(1)))   # one ulp above
    oh, ow = out_hw
    mask, area, cy, cx = mask_and_droplets(p.cuda(), thresh, (oh, ow), 1)
    ref512 = (p.numpy() > np.float32(0.3)).astype(np.uint8)
    ref = resize_nearest_cv2(ref512, ow, oh)
    assert np.array_equal(mask.cpu().numpy(), ref)
    assert int(area.sum()) == int(ref.sum())


def test_more_droplets_than_the_first_output_capacity():
    """The output arrays are sized for 65536 droplets; a mask with more (isolated pixels) takes the second pass."""
    from unet_dc_segmentation_amd.droplets import mask_and_droplets
    m = np.zeros((1024, 1024), np.float32)
    m[::2, ::2] = 1.0                                          # 262144 one-pixel objects
    mask, area, cy, cx = mask_and_droplets(torch.from_numpy(m).cuda(), 0.5, (1024, 1024), 1)
    assert len(area) == 262144 and int(area.min()) == 1 and int(area.max()) == 1
    assert cy[0] == 0 and cx[1] == 2 and cy[512] == 2 and cx[512] == 0          # raster order


# ---- what droplets.py launches: one body for the batch and the single image -------------------------------------------------
# Per image, for an output size that differs from the probabilities' (MASK_RESIZE "reference": the linear resize); at equal
# size the mask kernel is unetdc_mask_from_probs instead.  Recorded on the commit before the two launch paths became one.
LINEAR, CLEAN, PROPS = "unetdc_mask_from_probs_linear", "unetdc_mask_clean", "unetdc_label_props"
NEIGHBORS, CONFIDENCE, HULL = "unetdc_label_neighbors", "unetdc_label_confidence", "unetdc_label_hull"
# case: (options, the launches of one image, the device->host copies of one batch)
LAUNCHES = {
    "plain": (dict(), [LINEAR, "unetdc_ccl_stats"], 3),
    "split": (dict(split_depth=2.0), [LINEAR, "unetdc_split_stats"], 3),
    "shape": (dict(shape=True), [LINEAR, "unetdc_ccl_labels", PROPS], 3),
    "shape_gray": (dict(shape=True, gray=True), [LINEAR, "unetdc_ccl_labels", PROPS], 3),
    "labels_shape": (dict(shape=True, return_labels=True), [LINEAR, "unetdc_ccl_labels", PROPS], 3),
    "clean_low": (dict(thresh_low=0.3), [LINEAR, LINEAR, CLEAN, "unetdc_ccl_stats"], 3),
    "clean_holes": (dict(max_hole_area=-1), [LINEAR, CLEAN, "unetdc_ccl_stats"], 3),
    "all": (dict(split_depth=2.0, return_labels=True, shape=True, gray=True, thresh_low=0.3, max_hole_area=5),
            [LINEAR, LINEAR, CLEAN, "unetdc_split_stats", PROPS], 3),
    # the stages added since: recorded on the commit before they moved into the stage table
    "neighbors": (dict(neighbors=3), [LINEAR, "unetdc_ccl_labels", NEIGHBORS], 5),
    "confidence": (dict(confidence=0.1), [LINEAR, "unetdc_ccl_labels", CONFIDENCE], 3),
    "hull": (dict(hull=True), [LINEAR, "unetdc_ccl_labels", HULL], 3),
    "everything": (dict(split_depth=2.0, return_labels=True, shape=True, gray=True, thresh_low=0.3, max_hole_area=5, neighbors=3,
                        confidence=0.1, confidence_maps=True, hull=True),
                   [LINEAR, LINEAR, CLEAN, "unetdc_split_stats", PROPS, NEIGHBORS, CONFIDENCE, HULL], 5),
}


def disc_maps(n):
    """n 64 x 64 maps of discs (0.9) with skirts (0.4) and a one-pixel hole."""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:64, 0:64]
    p = np.full((n, 64, 64), 0.1, np.float32)
    for i in range(n):
        for _ in range(9):
            cy, cx, r = rng.integers(4, 60), rng.integers(4, 60), rng.integers(2, 8)
            d = (yy - cy) ** 2 + (xx - cx) ** 2
            p[i][(d <= (r + 2) ** 2) & (p[i] < 0.4)] = 0.4
            p[i][d <= r * r] = 0.9
        p[i, 30:33, 30:33] = 0.9
        p[i, 31, 31] = 0.1
    return p


@pytest.fixture(scope="module")
def launch_probs():
    return torch.from_numpy(disc_maps(2)).cuda()


@pytest.mark.parametrize("case", sorted(LAUNCHES))
def test_batch_and_single_image_launch_what_they_launched(case, launch_probs, monkeypatch):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.droplets import mask_and_droplets, mask_and_droplets_batch
    kw, linear, copies = LAUNCHES[case]
    kw, want = dict(kw), {"cpu": copies, "item": 0}
    equal = [n.replace("_linear", "") for n in linear]
    sizes = [(37, 53), (64, 96)]
    grays = {hw: torch.zeros(hw, dtype=torch.uint8, device="cuda") for hw in sizes + [(64, 64)]} if kw.pop("gray", False) else None
    names, real = [], _lib.call
    calls = {"cpu": 0, "item": 0}
    real_cpu, real_item = torch.Tensor.cpu, torch.Tensor.item

    def cpu(self, *a, **k):
        calls["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)

    def item(self):
        calls["item"] += self.is_cuda
        return real_item(self)

    def launched(fn, probs, hws, one):
        names.clear()
        calls.update(cpu=0, item=0)
        g = None if grays is None else grays[hws] if one else [grays[hw] for hw in hws]
        return fn(probs, 0.5, hws, 1, gray=g, **kw), list(names), dict(calls)
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    monkeypatch.setattr(torch.Tensor, "item", item)
    out, got, waits = launched(mask_and_droplets_batch, launch_probs, sizes, False)
    assert got == linear + linear and waits == want
    _, got, waits = launched(mask_and_droplets_batch, launch_probs[1:], [(64, 64)], False)
    assert got == equal and waits == want
    one, got, waits = launched(mask_and_droplets, launch_probs[0], sizes[0], True)
    assert got == linear and waits == want
    _, got, waits = launched(mask_and_droplets, launch_probs[1], (64, 64), True)
    assert got == equal and waits == want
    assert len(one.area) > 1 and (one.labels is not None) == kw.get("return_labels", False) and (one.props is not None) == ("shape" in kw)
    assert torch.equal(one.mask, out[0].mask) and all(np.array_equal(x, y) for x, y in zip(list(one)[1:], list(out[0])[1:]))


# ---- the optional stages share one int32 and one int64 allocation per batch: none may move another's numbers -------------------
STAGES = {"props": dict(shape=True), "neighbors": dict(neighbors=3), "confidence": dict(confidence=0.1), "hull": dict(hull=True)}


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    return type(a) is type(b) and np.array_equal(a, b)


@pytest.mark.parametrize("clean", [dict(), dict(thresh_low=0.3, max_hole_area=5)], ids=["raw", "clean"])
@pytest.mark.parametrize("split", [dict(), dict(split_depth=1.0)], ids=["ccl", "split"])
@pytest.mark.parametrize("B", [3, 2])
def test_every_subset_of_stages_leaves_each_stage_its_own_numbers(B, split, clean):
    """Every subset of the four stages that measure on the label map, with and without a split depth and cleaning, on batches
    of 3 and 2 images (both parities of the int32 region, so both states of the pad before the int64 totals): each stage's
    record equals, array by array, its record when it is the only stage on; mask, labels, areas, centroids and clean counts
    equal those runs' too.  Integer work, one device, the same kernels: no tolerance."""
    import itertools
    from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
    rng = np.random.default_rng(11)
    p = disc_maps(3)[:B]
    lo, hi = (p - rng.random(p.shape, dtype=np.float32) * np.float32(0.2), p + rng.random(p.shape, dtype=np.float32) * np.float32(0.2))
    probs, env = torch.from_numpy(p).cuda(), tuple(torch.from_numpy(e.astype(np.float32)).cuda() for e in (lo, hi))
    hws = [(37, 53), (64, 96), (64, 64)][:B]

    def run(fields):
        kw = dict(split, **clean)
        for f in fields:
            kw.update(STAGES[f])
        if "confidence" in fields:
            kw["envelope"] = env
        return mask_and_droplets_batch(probs, 0.5, hws, 1, return_labels=bool(fields or split), **kw)
    base = run(())
    alone = {f: run((f,)) for f in STAGES}
    assert min(len(d.area) for d in base) > 1
    for k in range(len(STAGES) + 1):
        for fields in itertools.combinations(STAGES, k):
            for i, d in enumerate(run(fields)):
                for f in STAGES:
                    got = getattr(d, f)
                    assert (got is None) if f not in fields else same(got, getattr(alone[f][i], f)), (fields, i, f)
                ref = alone[fields[0]][i] if fields else base[i]
                assert torch.equal(d.mask, ref.mask) and torch.equal(d.mask, base[i].mask), (fields, i)
                assert (d.labels is None and ref.labels is None) or torch.equal(d.labels, ref.labels), (fields, i)
                for name in ("area", "centroid_row", "centroid_col", "clean_counts"):
                    assert np.array_equal(getattr(d, name), getattr(ref, name)), (fields, i, name)
                    assert np.array_equal(getattr(d, name), getattr(base[i], name)), (fields, i, name)
            assert bool(clean) == bool(base[0].clean_counts.any())


def test_an_image_that_overflows_two_rooms_at_once_is_run_again_until_all_hold(monkeypatch):
    """Room for 4 droplets, 2 contact pairs and one row-extent slot per droplet: every image overflows the droplet capacity,
    then the pair lists and the row room, and comes out as with the default rooms."""
    from tests.test_gpu_hull import batch_inputs
    from unet_dc_segmentation_amd import droplets as D
    hws, p = batch_inputs()
    probs = torch.from_numpy(p).cuda()
    kw = dict(neighbors=3, hull=True, return_labels=True)
    want = D.mask_and_droplets_batch(probs, 0.5, hws, 2, **kw)
    names, real = [], D._lib.call
    monkeypatch.setattr(D, "PAIR_ROOM", 2)
    monkeypatch.setattr(D, "ROWS_PER_DROPLET", 1)
    monkeypatch.setattr(D._lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = D.mask_and_droplets_batch(probs, 0.5, hws, 2, max_droplets=4, **kw)
    assert names.count(NEIGHBORS) >= 2 * len(hws) and names.count(HULL) >= 2 * len(hws)
    assert max(len(w.neighbors["pairs"]["a"]) for w in want) > 2         # the last image: 7 pairs, so room for 2, 4, then 8
    for d, w in zip(got, want):
        assert len(w.area) > 4 and int(w.hull["nv"].max()) >= 3           # a droplet spans rows: more row slots than droplets
        assert same(d.neighbors, w.neighbors) and same(d.hull, w.hull) and torch.equal(d.labels, w.labels)
        assert np.array_equal(d.area, w.area)


# ---- unetdc_ccl_stats and the mask kernels through the C ABI, every output and the workspace (at exactly
# unetdc_ccl_workspace bytes) between canaries ----------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ccl_canaried(m, min_area, max_out=None):
    """-> (count, area, sum_row, sum_col, root: int64 arrays of min(count, max_out) entries).  The per-droplet outputs hold
    exactly max_out entries, so the canary begins at entry max_out."""
    from unet_dc_segmentation_amd import _lib
    h, w = m.shape
    nbytes = _lib.load().unetdc_ccl_workspace(h, w)
    cap = h * w if max_out is None else max_out
    mask = torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8)).cuda()
    ws, count = Canaried(nbytes), Canaried(4)
    area, root, sy, sx = Canaried(4 * cap), Canaried(4 * cap), Canaried(8 * cap), Canaried(8 * cap)
    _lib.call("unetdc_ccl_stats", mask.data_ptr(), h, w, min_area, ws.ptr, nbytes, count.ptr, area.ptr, sy.ptr, sx.ptr, root.ptr,
              cap, _stream())
    torch.cuda.synchronize()
    for v, what in ((ws, "workspace"), (count, "count"), (area, "areas"), (root, "roots"), (sy, "row sums"), (sx, "column sums")):
        v.check("ccl " + what)
    assert np.array_equal(mask.cpu().numpy(), m)
    n = int(count.numpy(np.int32, 1)[0])
    k = min(n, cap)
    cols = [area.numpy(np.int32, cap), sy.numpy(np.int64, cap), sx.numpy(np.int64, cap), root.numpy(np.int32, cap)]
    for v in cols:                                                     # entries at min(count, max_out) and above: untouched
        assert np.all(v[k:].view(np.uint8) == 0xA5)
    return (n,) + tuple(v[:k].astype(np.int64) for v in cols)


def _scipy_table(m, min_area):
    """(area, sum_row, sum_col, first raster index) per 4-connected component of at least min_area pixels, as int64, in
    scipy.ndimage.label's order (raster order of the first pixel)."""
    lab, n = ndimage.label(m)                                          # the default structure: 4-connectivity
    flat = lab.ravel()
    area = np.bincount(flat, minlength=n + 1)[1:].astype(np.int64)
    yy, xx = np.divmod(np.arange(flat.size, dtype=np.int64), m.shape[1])
    sy = np.bincount(flat, weights=yy, minlength=n + 1)               # float64 sums of integers below 2^53: exact
    sx = np.bincount(flat, weights=xx, minlength=n + 1)
    assert sy.max(initial=0) < 2.0 ** 53 and sx.max(initial=0) < 2.0 ** 53
    sy, sx = sy.astype(np.int64), sx.astype(np.int64)
    first = np.full(n + 1, flat.size, np.int64)
    idx = np.flatnonzero(flat)[::-1]
    first[flat[idx]] = idx                                             # the last write is the smallest index
    assert np.all(np.diff(first[1:]) > 0)                              # label order IS raster order of the first pixel
    keep = area >= min_area
    return area[keep], sy[1:][keep], sx[1:][keep], first[1:][keep]


def _assert_ccl_matches_scipy(m, min_area, max_out=None, want=None):
    n, area, sy, sx, root = _ccl_canaried(m, min_area, max_out)
    want = _scipy_table(m, min_area) if want is None else want
    assert n == len(want[0])                                           # the full count, whatever max_out
    k = len(area)
    assert k == (n if max_out is None else min(n, max_out))
    for got, w, what in zip((area, sy, sx, root), want, ("area", "row sum", "column sum", "first pixel")):
        assert got.dtype == np.int64 and np.array_equal(got, w[:k]), what
    return n


CCL_SHAPES = [(1, 4097), (4097, 1), (1, 1), (700, 1), (512, 2), (341, 3), (205, 5), (33, 31), (32, 32), (25, 41), (1, 1023),
              (1, 1024), (1025, 1), (1040, 1388), (2048, 2048)]


@pytest.mark.parametrize("min_area", [1, 3])
@pytest.mark.parametrize("shape", CCL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ccl_stats_geometry_against_scipy(shape, min_area):
    """One-row, one-column and one-pixel masks; widths 1, 2, 3 and 5 (ccl_emit_kernel's 4 pixels per thread straddle row
    ends); n = 1023, 1024, 1025 around the 1024-pixel scan block; 1410 and 4096 scan blocks (ccl_scan_kernel with 2 and 4
    trips of 1024 block sums).  Random masks near the 4-connected site-percolation threshold (0.593)."""
    h, w = shape
    m = (np.random.default_rng(h * 3 + w).random((h, w)) < 0.58).astype(np.uint8)
    want = _scipy_table(m, min_area)
    n = _assert_ccl_matches_scipy(m, min_area, want=want)
    assert n >= 1 or h * w == 1
    if h * w >= 1023:
        _assert_ccl_matches_scipy(m, min_area, max_out=max(n // 2, 1), want=want)


EMIT_ROOTS = (0, 3, 4, 255 * 4 + 3, 1024, 2047)


@pytest.mark.parametrize("shape", [(1, 2048), (1024, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ccl_emit_ranks_at_the_thread_and_block_seams(shape):
    """ccl_emit_kernel ranks the kept roots by a workgroup scan of 256 per-thread counts, four pixels a thread, 1024 a block.
    Pixels 0, 3, 4, 1023, 1024 and 2047 set: the first and the last pixel of thread 0, the first of thread 1, the last of block
    0, the first and the last of block 1.  As 1024 x 2 no two of them are 4-neighbours and each is a root (a thread holds 0, 1
    or 2 roots, the most a 4-connected mask allows); as 1 x 2048 the pairs 3|4 and 1023|1024 unite into objects of two
    pixels.  The chessboard (every pixel a root, two a thread) is test_ccl_table_matches_scipy[checker]."""
    m = np.zeros(2048, np.uint8)
    m[list(EMIT_ROOTS)] = 1
    m = m.reshape(shape)
    want = _scipy_table(m, 1)
    assert want[3].tolist() == (list(EMIT_ROOTS) if shape[1] == 2 else [0, 3, 1023, 2047])
    assert _assert_ccl_matches_scipy(m, 1, want=want) == len(want[3])
    _assert_ccl_matches_scipy(m, 1, max_out=3, want=want)
    if shape[1] != 2:
        assert _assert_ccl_matches_scipy(m, 2) == 2


@pytest.mark.parametrize("value", [0, 1])
def test_ccl_stats_single_pixel(value):
    n, area, sy, sx, root = _ccl_canaried(np.full((1, 1), value, np.uint8), 1)
    assert n == value and list(area) == [1] * value and list(root) == [0] * value


@pytest.mark.parametrize("min_area", [2, 5])
def test_ccl_stats_min_area_boundary(min_area):
    """Components of exactly min_area - 1, min_area and min_area + 1 pixels: the first are dropped, the others kept."""
    m = fx.area_boundary_mask(min_area)
    n, area, sy, sx, root = _ccl_canaried(m, min_area)
    assert n == 6 and sorted(area) == [min_area] * 3 + [min_area + 1] * 3
    _assert_ccl_matches_scipy(m, min_area)
    _assert_ccl_matches_scipy(m, min_area, max_out=4)
    assert _assert_ccl_matches_scipy(m, 1) == 9


def test_ccl_stats_max_out_zero_and_workspace_too_small():
    from unet_dc_segmentation_amd import _lib
    m = fx.area_boundary_mask(2)
    assert _assert_ccl_matches_scipy(m, 1, max_out=0) == 9
    h, w = m.shape
    nbytes = _lib.load().unetdc_ccl_workspace(h, w)
    mask = torch.from_numpy(m).cuda()
    ws, outs = Canaried(nbytes), [Canaried(4), Canaried(4 * 16), Canaried(8 * 16), Canaried(8 * 16), Canaried(4 * 16)]
    rc = _lib.load().unetdc_ccl_stats(mask.data_ptr(), h, w, 1, ws.ptr, nbytes - 1, *[o.ptr for o in outs], 16, _stream())
    torch.cuda.synchronize()
    assert rc == -3                                                    # UNETDC_EWORKSPACE, before any launch
    assert ws.untouched() and all(o.untouched() for o in outs)


def _special_probs(h, w, seed):
    p = np.random.default_rng(seed).random((h, w)).astype(np.float32)
    flat = p.ravel()
    for j, v in enumerate([np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0, -0.5, np.nextafter(np.float32(1), np.float32(2)),
                           np.nextafter(np.float32(0), np.float32(1)), -np.nan]):
        flat[j::17][:max(1, flat.size // 40)] = v
    return p


@pytest.mark.parametrize("thresh", [0.0, 1.0, -0.5, 0.3])
@pytest.mark.parametrize("out_hw", [(37, 53), (53, 37), (90, 11), (1, 1)])
def test_mask_from_probs_special_values_and_thresholds(out_hw, thresh):
    """NaN compares false, +inf true, -inf false; thresholds 0, 1 and a negative one.  Reference: p > np.float32(t) in numpy,
    then cv2's nearest-neighbour index rule."""
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.droplets import resize_nearest_cv2
    ph, pw = 37, 53
    p = _special_probs(ph, pw, 3)
    oh, ow = out_hw
    with np.errstate(invalid="ignore"):
        want = resize_nearest_cv2((p > np.float32(thresh)).astype(np.uint8), ow, oh)
    out, pd = Canaried(oh * ow), torch.from_numpy(p).cuda()
    _lib.call("unetdc_mask_from_probs", pd.data_ptr(), ph, pw, float(thresh), out.ptr, oh, ow, _stream())
    torch.cuda.synchronize()
    out.check("mask")
    got = out.numpy(np.uint8, oh, ow)
    assert np.array_equal(got, want)
    assert 0 < int(want.sum()) < want.size or oh * ow == 1


@pytest.mark.parametrize("p_hw,out_hw", [((1, 64), (40, 97)), ((64, 1), (97, 40)), ((1, 64), (1, 200)), ((64, 1), (200, 1)),
                                         ((48, 64), (1, 97)), ((48, 64), (97, 1)), ((1, 1), (9, 13))])
def test_mask_from_probs_linear_one_row_and_one_column(p_hw, out_hw):
    """1 x W and H x 1 probability maps (and outputs): the reference's 8-bit INTER_LINEAR on the thresholded mask."""
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.preprocess import _resize_tables
    from utils.data_loader import resize_linear_cv2_u8
    (ph, pw), (oh, ow) = p_hw, out_hw
    p = _special_probs(ph, pw, 5) if ph * pw > 1 else np.full((1, 1), 0.7, np.float32)
    thresh = np.float32(0.4)
    with np.errstate(invalid="ignore"):
        want = resize_linear_cv2_u8((p > thresh).astype(np.uint8), ow, oh)
    dev = torch.device("cuda", torch.cuda.current_device())
    xo, xa = _resize_tables(pw, ow, dev, True)
    yo, ya = _resize_tables(ph, oh, dev, False)
    out, pd = Canaried(oh * ow), torch.from_numpy(p).cuda()
    _lib.call("unetdc_mask_from_probs_linear", pd.data_ptr(), ph, pw, float(thresh), out.ptr, oh, ow,
              xo.data_ptr(), xa.data_ptr(), yo.data_ptr(), ya.data_ptr(), _stream())
    torch.cuda.synchronize()
    out.check("mask")
    assert np.array_equal(out.numpy(np.uint8, oh, ow), want)
