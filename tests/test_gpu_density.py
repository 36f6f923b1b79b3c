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
    a = density_maps_batch(rgbs, [o[0] for o in out], sums, 10, 21)
    b = density_maps_batch(rgbs, [o[0] for o in out], None, 10, 21)
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
