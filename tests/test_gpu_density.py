"""GPU: the density-map kernels (csrc/density.hip) stage by stage against the host restatement utils/density.py, bit for bit,
and quantify_droplets_batch.py --density_maps on the device against the same restatement."""
import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from utils import density as hd

pytestmark = pytest.mark.gpu


def _cases():
    import bench
    from tests.test_density_cpu import cell_image
    im = bench.synthetic_micrograph(7)
    yield "micrograph_1040x1388", im, (hd.rgb_to_gray(im) > 110).astype(np.uint8)
    yield "cell_600x800", *cell_image(600, 800, 3)
    yield "odd_37x1001", *cell_image(37, 1001, 4)
    yield "odd_1001x37", *cell_image(1001, 37, 5)
    rgb = np.random.default_rng(0).integers(0, 256, (2, 2, 3)).astype(np.uint8)
    yield "smallest_2x2", rgb, np.array([[1, 0], [0, 1]], np.uint8)
    yield "no_droplets_64x80", cell_image(64, 80, 6)[0], np.zeros((64, 80), np.uint8)
    yield "flat_image_50x50", np.full((50, 50, 3), 77, np.uint8), cell_image(50, 50, 7)[1]
    from tests.test_density_cpu import stripe_image
    m = np.zeros((8, 108), np.uint8)
    m[2:4, 10:14] = m[5, 60] = m[1:7, 95] = 1
    yield "otsu_tie_stripes_8x108", stripe_image(), m


CASES = list(_cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("layers,kernel", [(10, 21), (255, 55), (1, 6)])
def test_every_stage_bit_exact(case, layers, kernel):
    from unet_dc_segmentation_amd.density import density_maps_batch
    _, rgb, mask = case
    ref = hd.density_maps(rgb, mask, layers, kernel)
    dev = density_maps_batch([torch.from_numpy(rgb).cuda()], [torch.from_numpy(mask).cuda()], None, layers, kernel,
                             planes=True)[0]
    for k in ("blur", "roi", "ring"):
        assert np.array_equal(dev[k].cpu().numpy(), ref[k]), k
    assert dev["threshold"] == ref["threshold"]
    assert (dev["roi_area"], dev["cx"], dev["cy"]) == (ref["roi_area"], ref["cx"], ref["cy"])
    assert dev["max_ring_distance"] == ref["max_ring_distance"]
    assert np.array_equal(dev["ring_counts"], ref["ring_counts"])
    for k in ("radial", "spatial"):
        d = dev[k].cpu().numpy()
        assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), ref[k].view(np.uint32)), k
    for k in ("radial_index", "spatial_index"):
        assert np.array_equal(dev[k], ref[k]), k


def test_batch_reuses_droplet_sums_and_matches_single_images():
    from unet_dc_segmentation_amd.density import density_maps_batch
    from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
    from tests.test_density_cpu import cell_image
    imgs = [cell_image(96, 128, 20), cell_image(96, 128, 21)]
    probs = torch.stack([torch.from_numpy(m.astype(np.float32)) for _, m in imgs]).cuda()
    out, sums = mask_and_droplets_batch(probs, 0.5, [(96, 128)] * 2, 1, keep_sums=True)
    assert sums is not None
    rgbs = [torch.from_numpy(r).cuda() for r, _ in imgs]
    a = density_maps_batch(rgbs, [o.mask for o in out], sums, 10, 21)
    b = density_maps_batch(rgbs, [o.mask for o in out], None, 10, 21)
    for x, y, (rgb, m) in zip(a, b, imgs):
        ref = hd.density_maps(rgb, m, 10, 21)
        for k in ("radial_index", "spatial_index"):
            assert np.array_equal(x[k], ref[k]) and np.array_equal(y[k], ref[k])
        assert np.array_equal(x["ring_counts"], ref["ring_counts"]) and x["ndroplets"] == y["ndroplets"]


def test_device_sqrt_of_every_distance_squared():
    from unet_dc_segmentation_amd.density import density_sqrt
    k = torch.arange(0, 1040 ** 2 + 1388 ** 2 + 1, dtype=torch.int64, device="cuda")
    got = density_sqrt(k).cpu().numpy()
    ref = np.sqrt(np.arange(0, 1040 ** 2 + 1388 ** 2 + 1, dtype=np.int64).astype(np.float64))
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_cli_density_maps_on_device(tmp_path):
    import quantify_droplets_batch as q
    from models.model_2 import UNetDC
    from tests.test_density_cpu import cell_image
    assert q.DEVICE == "cuda"
    import bench
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    sizes = [(1040, 1388), (300, 401), (96, 96), (37, 1001), (512, 512), (200, 150), (64, 640), (1040, 1388)]
    for i, (h, w) in enumerate(sizes):
        im = bench.synthetic_micrograph(30 + i) if (h, w) == (1040, 1388) else cell_image(h, w, 30 + i)[0]
        Image.fromarray(im).save(img_dir / f"im{i}.png")
    torch.manual_seed(0)
    m = UNetDC(3, 1)
    with torch.no_grad():
        m.out_conv.bias += 2.0                       # a few droplets even from random weights
    torch.save(m.state_dict(), tmp_path / "ck.pth")
    out = tmp_path / "out"
    q.main(["--img_dir", str(img_dir), "--ckpt_path", str(tmp_path / "ck.pth"), "--out_dir", str(out), "--batch", "8",
            "--skip_excel", "--skip_histogram", "--density_maps"])
    csv = pd.read_csv(out / "density_per_image.csv", float_precision="round_trip")
    assert len(csv) == 8
    lut = hd.colormap_lut("hot")
    for i in range(8):
        rgb = np.array(Image.open(img_dir / f"im{i}.png").convert("RGB"))
        mask = (np.array(Image.open(out / "predicted_masks" / f"im{i}_pred.png")) > 0).astype(np.uint8)
        r = hd.density_maps(rgb, mask, 10, 21)
        row = csv.iloc[i]
        exp = hd.csv_row(f"im{i}.png", r, 10)
        assert {k: row[k] for k in exp} == exp
        for k in ("radial", "spatial"):
            assert np.array_equal(np.array(Image.open(out / f"im{i}_{k}_density.png")), lut[r[f"{k}_index"]]), (i, k)


# ---- unetdc_density_maps through the C ABI ----------------------------------------------------------------------------------
PLANES = (("blur", np.uint8), ("roi", np.uint8), ("ring", np.uint8), ("radial", np.float32), ("spatial", np.float32))


def device_density(rgb, mask, layers, kernel, table=None, max_droplets=None, planes=True, ws=None):
    """One unetdc_density_maps call -> dict: "stats" (the unetdc_density_stats record as a numpy record), "stats_bytes" (its
    1088 bytes), radial_index, spatial_index, and with planes=True the five optional planes (NULL otherwise).  table: (area,
    sum of rows, sum of columns) of the droplets, by default those of the mask's components; max_droplets: how many entries
    the call may read (all by default; the arrays hold exactly that many, between canaries).  Every output and the workspace
    (a Canaried view of exactly the queried bytes, `ws` when the test prepared one) sit between canaries."""
    from tests.image_canaries import Canaried, canaried_like
    from tests.workspace_states import droplet_table
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.density import STATS_DTYPE
    lib = _lib.load()
    h, w = mask.shape
    area, sy, sx = droplet_table(mask) if table is None else table
    n = len(area)
    cap = n if max_droplets is None else max_droplets
    k = min(n, cap)
    cnt = canaried_like(np.array([n], np.int32))
    d_area, d_sy, d_sx = (canaried_like(np.ascontiguousarray(v[:k], dtype=t)) for v, t in ((area, np.int32), (sy, np.int64), (sx, np.int64)))
    nbytes = lib.unetdc_density_workspace(h, w)
    if ws is None:
        ws = Canaried(nbytes)
    assert ws.nbytes == nbytes > 0
    d_rgb = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
    d_mask = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    st = Canaried(STATS_DTYPE.itemsize)
    ri, si = Canaried(h * w), Canaried(h * w)
    opt = {name: Canaried(h * w * np.dtype(t).itemsize) for name, t in PLANES} if planes else {}
    taps = hd.gaussian_taps(kernel / 6)
    _lib.call("unetdc_density_maps", d_rgb.data_ptr(), d_mask.data_ptr(), h, w, cnt.ptr, d_area.ptr, d_sy.ptr, d_sx.ptr, cap,
              int(layers), float(kernel / 6), taps.ctypes.data, ws.ptr, nbytes, st.ptr, ri.ptr, si.ptr,
              *(opt[name].ptr if planes else None for name, _ in PLANES), torch.cuda.current_stream().cuda_stream)
    for name, v in (("workspace", ws), ("stats", st), ("radial_index", ri), ("spatial_index", si), ("count", cnt), ("area", d_area),
                    ("sumy", d_sy), ("sumx", d_sx), *opt.items()):
        v.check(name)
    assert cnt.numpy(np.int32, 1)[0] == n and np.array_equal(d_area.numpy(np.int32, k), area[:k])       # the inputs are read only
    sb = st.numpy(np.uint8, STATS_DTYPE.itemsize).copy()
    out = {"stats_bytes": sb, "stats": sb.view(STATS_DTYPE)[0], "radial_index": ri.numpy(np.uint8, h, w),
           "spatial_index": si.numpy(np.uint8, h, w)}
    out.update((name, opt[name].numpy(t, h, w)) for name, t in PLANES if planes)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_density_equals_host(dev, ref, layers, ndroplets, planes=True):
    """Every field of the record, the two index planes and (when given) the five optional planes against the dict of
    utils.density.density_maps (ring_counts possibly replaced by the caller)."""
    st = dev["stats"]
    assert (int(st["otsu_threshold"]), int(st["roi_area"]), int(st["cx"]), int(st["cy"])) == (ref["threshold"], ref["roi_area"], ref["cx"], ref["cy"])
    ys, xs = np.nonzero(ref["roi"])
    assert (int(st["m10"]), int(st["m01"])) == (int(xs.sum()), int(ys.sum()))
    assert int(st["nb_layers"]) == layers and int(st["ndroplets"]) == ndroplets
    assert np.float64(st["max_ring_distance"]).view(np.uint64) == np.float64(ref["max_ring_distance"]).view(np.uint64)
    assert np.array_equal(st["ring_count"][:layers], ref["ring_counts"]) and not st["ring_count"][layers:].any()
    for k in ("radial", "spatial"):
        assert int(st[f"{k}_min_bits"]) == int(bits(ref[k]).min()) and int(st[f"{k}_max_bits"]) == int(bits(ref[k]).max()), k
        assert np.array_equal(dev[f"{k}_index"], ref[f"{k}_index"]), k
        if planes:
            assert dev[k].dtype == np.float32 and np.array_equal(bits(dev[k]), bits(ref[k])), k
    if planes:
        for k in ("blur", "roi", "ring"):
            assert np.array_equal(dev[k], ref[k]), k


def host_with_table(rgb, mask, layers, kernel, table, cap):
    """utils.density.density_maps with the ring counts, the radial map and its index plane of a droplet table of which only
    the first `cap` entries count (the ring rule of utils.density.radial_map on the truncated table)."""
    ref = hd.density_maps(rgb, mask, layers, kernel)
    a = np.asarray(table[0][:cap], dtype=np.float64)
    cen = (np.asarray(table[1][:cap], dtype=np.float64) / a, np.asarray(table[2][:cap], dtype=np.float64) / a)
    radial, ring, counts, maxd = hd.radial_map(mask, ref["roi"], layers, ref["cy"], ref["cx"], centroids=cen)
    assert np.array_equal(ring, ref["ring"]) and maxd == ref["max_ring_distance"]
    ref.update(ring_counts=counts, radial=radial, radial_index=hd.colormap_index(radial))
    return ref


def droplet_table_of(mask):
    from tests.workspace_states import droplet_table
    return droplet_table(mask)[0]


def test_abi_max_droplets_below_the_count_reads_the_first_entries_only():
    from tests.droplet_edge_fixtures import ring_counts_of_table
    from tests.test_density_cpu import cell_image
    from tests.workspace_states import droplet_table
    rgb, mask = cell_image(96, 130, 11)
    mask = mask | (np.random.default_rng(11).random(mask.shape) < 0.02).astype(np.uint8)      # a few hundred droplets
    table = droplet_table(mask)
    n = len(table[0])
    full = hd.density_maps(rgb, mask, 10, 21)
    assert n > 100 and full["ring_counts"].sum() > 40
    seen = []
    for cap in (n, 150, 60, 20, 0):
        ref = host_with_table(rgb, mask, 10, 21, table, cap)
        assert np.array_equal(ref["ring_counts"], ring_counts_of_table(*table, cap, ref["roi"], 10))
        assert ref["ring_counts"].sum() <= cap and ref["ring_counts"].tolist() not in seen      # every capacity: other counts
        seen.append(ref["ring_counts"].tolist())
        dev = device_density(rgb, mask, 10, 21, table, max_droplets=cap)
        assert_density_equals_host(dev, ref, 10, n)                        # ndroplets: the full count whatever the capacity
    assert np.array_equal(host_with_table(rgb, mask, 10, 21, table, n)["ring_counts"], full["ring_counts"])


def test_abi_droplets_on_ring_bounds_belong_to_the_lower_ring_and_the_centroid_to_none():
    from tests.droplet_edge_fixtures import BOUND_LAYERS, bound_case
    rgb, mask, rings, counts = bound_case()
    ref = hd.density_maps(rgb, mask, BOUND_LAYERS, 21)
    assert (ref["cx"], ref["cy"], ref["max_ring_distance"], ref["roi_area"]) == (80, 60, 100.0, mask.size)
    assert np.array_equal(ref["ring_counts"], counts) and counts.sum() == len(rings) - 1       # the droplet at the centroid: none
    dev = device_density(rgb, mask, BOUND_LAYERS, 21)
    assert_density_equals_host(dev, ref, BOUND_LAYERS, len(rings))
    assert dev["roi"][60, 80] == 1 and dev["ring"][60, 80] == 0 and dev["radial"][60, 80] == 0.0   # the ROI pixel at the centroid
    assert dev["ring"][60, 90] == 1 and dev["ring"][60, 91] == 2 and dev["ring"][0, 0] == BOUND_LAYERS   # pixels on b_1, past it, on b_L


def test_abi_255_layers_on_a_small_image():
    from tests.test_density_cpu import cell_image
    rgb, mask = cell_image(64, 80, 6)
    ref = hd.density_maps(rgb, mask, 255, 21)
    assert ref["roi_area"] > 0 and ref["ring_counts"].sum() > 0 and (ref["ring_counts"] == 0).sum() > 200     # most rings empty
    dev = device_density(rgb, mask, 255, 21)
    assert_density_equals_host(dev, ref, 255, len(droplet_table_of(mask)))


@pytest.mark.parametrize("shape,layers", [((96, 130), 10), ((37, 53), 255)])
def test_abi_optional_planes_null_or_given_same_bytes(shape, layers):
    from tests.test_density_cpu import cell_image
    rgb, mask = cell_image(*shape, 12)
    ref = hd.density_maps(rgb, mask, layers, 21)
    given = device_density(rgb, mask, layers, 21, planes=True)
    null = device_density(rgb, mask, layers, 21, planes=False)
    assert_density_equals_host(given, ref, layers, len(droplet_table_of(mask)))
    assert_density_equals_host(null, ref, layers, len(droplet_table_of(mask)), planes=False)
    assert np.array_equal(given["stats_bytes"], null["stats_bytes"])
    for k in ("radial_index", "spatial_index"):
        assert np.array_equal(given[k], null[k]), k
