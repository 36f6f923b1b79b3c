"""GPU: the device-resident training data path (unet_dc_segmentation_amd/device_data.py, train_DC_focal.py --device_data)
against the host path (SegmentationDataset / DataLoader) on PNG files: 1040 x 1388 micrographs, one 276 x 408 image and one
grayscale PNG."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

N_PAIRS = 32


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    import bench
    d = tmp_path_factory.mktemp("device_data")
    ind, md = d / "images", d / "masks"
    ind.mkdir()
    md.mkdir()
    for i in range(N_PAIRS):
        if i == 1:
            img = bench.synthetic_micrograph(100 + i, h=276, w=408, discs=40)
        else:
            img = bench.synthetic_micrograph(100 + i % 5)
            if i % 5 != 0:
                img = np.roll(img, 37 * i, axis=1)
        mask = (img[..., 0] > 110).astype(np.uint8) * 255
        if i == 2:
            Image.fromarray(img[..., 0]).save(ind / f"img_{i:03d}.png")              # grayscale file
        else:
            Image.fromarray(img).save(ind / f"img_{i:03d}.png")
        Image.fromarray(mask).save(md / f"img_{i:03d}.png")
    return str(ind), str(md)


NAMES = ["img_001.png", "img_002.png", "img_000.png", "img_003.png", "img_007.png"]


@pytest.fixture(scope="module")
def cache(data_dir):
    from unet_dc_segmentation_amd.device_data import DeviceImageCache
    return DeviceImageCache(data_dir[0], data_dir[1], NAMES, 512, 50, "cuda")


def test_cache_matches_segmentation_dataset(data_dir, cache):
    from utils.data_loader import SegmentationDataset
    ds = SegmentationDataset(data_dir[0], data_dir[1], NAMES, NAMES)
    for i in range(len(NAMES)):
        img, mask, hw, name = ds[i]
        assert torch.equal(cache.images[i].cpu(), img), name
        assert torch.equal(cache.masks[i].cpu().float()[None], mask), name
        assert cache.orig_sizes[i] == hw and cache.names[i] == name
        assert cache.img_max[i] == float(img.max())


def test_eval_loader_matches_collated_dataset(data_dir, cache):
    from torch.utils.data import DataLoader

    from unet_dc_segmentation_amd.device_data import DeviceEvalLoader
    from utils.data_loader import SegmentationDataset
    ds = SegmentationDataset(data_dir[0], data_dir[1], NAMES, NAMES)
    got, want = list(DeviceEvalLoader(cache, 2)), list(DataLoader(ds, batch_size=2, shuffle=False))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert torch.equal(g[0].cpu(), w[0]) and torch.equal(g[1].cpu(), w[1])
        assert torch.equal(g[2][0], w[2][0]) and torch.equal(g[2][1], w[2][1]) and list(g[3]) == list(w[3])


def test_train_loader_deterministic_per_seed_and_epoch(cache):
    from unet_dc_segmentation_amd.device_data import DeviceTrainLoader
    a, b = DeviceTrainLoader(cache, 2, seed=3), DeviceTrainLoader(cache, 2, seed=3)
    ea = [[[t.cpu() for t in batch[:2]] for batch in a] for _ in range(2)]
    eb = [[[t.cpu() for t in batch[:2]] for batch in b] for _ in range(2)]
    assert len(ea[0]) == 3 and ea[0][-1][0].shape == (1, 3, 512, 512)
    for x, y in zip(ea, eb):
        for bx, by in zip(x, y):
            assert torch.equal(bx[0], by[0]) and torch.equal(bx[1], by[1])
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(ea[0], ea[1]))
    for batch in ea[0]:
        assert batch[0].min() >= 0 and batch[0].max() <= 1 and set(batch[1].unique().tolist()) <= {0.0, 1.0}


def _argv(data_dir, tmp_path, *extra):
    return ["--image_dir", data_dir[0], "--mask_dir", data_dir[1], "--ckpt_path", str(tmp_path / "ck.pth"), "--workers", "0",
            "--batch", "4", *extra]


def test_epochs_0_same_test_evaluation(data_dir, tmp_path):
    import train_DC_focal
    h_dev = train_DC_focal.main(_argv(data_dir, tmp_path, "--epochs", "0", "--dtype", "f32", "--device_data"))
    h_cpu = train_DC_focal.main(_argv(data_dir, tmp_path, "--epochs", "0", "--dtype", "f32"))
    assert h_dev.test is not None and h_dev.test == h_cpu.test


def test_device_data_trains_end_to_end(data_dir, tmp_path):
    import train_DC_focal
    h = train_DC_focal.main(_argv(data_dir, tmp_path, "--device_data", "--dtype", "bf16", "--epochs", "2", "--patience", "5"))
    assert len(h) == 2
    for rec in h:
        assert all(math.isfinite(rec[k]) for k in ("train_loss", "val_loss", "train_dice", "val_dice"))
        assert rec["images_per_sec"] > 0
    assert h.test is not None and math.isfinite(h.test["test_loss"])
    assert os.path.exists(tmp_path / "ck.pth") or h[0]["val_dice"] == 0
