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


# ---- loader parity: every sample of a DeviceTrainLoader batch against the host restatement of its own draw ---------------------
N_SMALL, SMALL_SIDE, SMALL_RADIUS = 40, 64, 9
# the loader's elastic settings on the small cache: displacements of about a pixel on a 64 x 64 image (the training defaults,
# sigma 50 and alpha 1, move nothing there).  The host fields differ from the device's by at most 1e-5 max|d| (the bound of
# tests/test_gpu_augment.py), about 1e-5 pixels here: inside the 5e-5 image tolerance and far inside the 1e-3 near-tie band.
SMALL_SIGMA, SMALL_ALPHA = 4.0, 8.0


@pytest.fixture(scope="module")
def small_cache(tmp_path_factory):
    """40 images of 64 x 64, written as PNGs like data_dir's: enough for one batch of more than 32."""
    import bench

    from unet_dc_segmentation_amd.device_data import DeviceImageCache
    d = tmp_path_factory.mktemp("device_data_small")
    ind, md = d / "images", d / "masks"
    ind.mkdir()
    md.mkdir()
    names = [f"s_{i:03d}.png" for i in range(N_SMALL)]
    for i, name in enumerate(names):
        img = bench.synthetic_micrograph(500 + i, h=SMALL_SIDE, w=SMALL_SIDE, discs=12)
        Image.fromarray(img).save(ind / name)
        Image.fromarray((img[..., 0] > 110).astype(np.uint8) * 255).save(md / name)
    return DeviceImageCache(str(ind), str(md), names, SMALL_SIDE, SMALL_RADIUS, "cuda")


def _assert_batch_matches_host(loader, host, epoch, idx, batch):
    """batch == [augment_ref.augment_with_params(cache image, cache mask, draw_params(seed, epoch, ids[i]), fields of that
    draw's field_seed) for i in idx]: bit-exact without elastic, the elastic tolerances of tests/test_gpu_augment.py with it.
    -> the number of elastic samples."""
    from tests import augment_ref as ref
    from tests import image_edge_fixtures as fx
    from unet_dc_segmentation_amd.augment import draw_params
    himg, hmask = host
    s = loader.dataset.size
    oi, om = batch[0].cpu().numpy(), batch[1].cpu().numpy()
    assert oi.shape == (len(idx), 3, s, s) and om.shape == (len(idx), 1, s, s)
    nel = 0
    for j, i in enumerate(idx):
        p = draw_params(loader.seed, epoch, loader.ids[i])
        dx = dy = None
        if p["elastic"]:
            dx, dy = ref.fields(p["field_seed"], s, s, loader.sigma, loader.alpha)
            nel += 1
        ei, em = ref.augment_with_params(himg[i].transpose(1, 2, 0), hmask[i], p, dx, dy)
        ei, em = ei.transpose(2, 0, 1), em.astype(np.float32)[None]
        what = (epoch, j, int(i), p)
        if not p["elastic"]:
            assert np.array_equal(oi[j].view(np.uint32), ei.view(np.uint32)), what
            assert np.array_equal(om[j], em), what
            continue
        assert np.abs(oi[j] - ei).max() <= 5e-5, (what, np.abs(oi[j] - ei).max())
        tie = fx.near_tie(dx, dy)
        assert tie.mean() <= fx.NEAR_TIE_CAP, (what, tie.mean())
        diff = om[j][0] != em[0]
        assert not (diff & ~tie).any(), (what, int(diff.sum()), int(tie.sum()))
    return nel


def _host(c):
    return c.images.cpu().numpy(), c.masks.cpu().numpy()


def _two_epochs_match_host(loader):
    host = _host(loader.dataset)
    nel = nbc = 0
    for epoch in range(2):
        perm = np.random.default_rng([loader.seed, epoch]).permutation(len(loader.dataset))
        batches = list(loader)                                      # the loader's own iteration: epoch, order and tail batch
        assert len(batches) == len(loader)
        for b, batch in enumerate(batches):
            idx = perm[b * loader.batch_size:(b + 1) * loader.batch_size]
            assert list(batch[3]) == [loader.dataset.names[i] for i in idx]
            nel += _assert_batch_matches_host(loader, host, epoch, idx, batch)
    return nel


def test_train_loader_batches_of_2_match_the_host_restatement(cache):
    """The module's 512 x 512 cache at the training defaults (sigma 50, alpha 1), two epochs."""
    from unet_dc_segmentation_amd.device_data import DeviceTrainLoader
    assert _two_epochs_match_host(DeviceTrainLoader(cache, 2, seed=3)) >= 1


@pytest.mark.parametrize("batch", [2, 36])
def test_train_loader_small_cache_matches_the_host_restatement(small_cache, batch):
    """36 > AUG_MAX_BATCH: the first batch of each epoch takes two gather launches; the tail batch has 4 samples."""
    from unet_dc_segmentation_amd.device_data import DeviceTrainLoader
    loader = DeviceTrainLoader(small_cache, batch, seed=11, sigma=SMALL_SIGMA, alpha=SMALL_ALPHA)
    assert _two_epochs_match_host(loader) >= 10


def test_train_loader_shard_draws_by_global_index(small_cache):
    """ids given (a data-parallel rank's shard of a larger split): sample i draws from (seed, epoch, ids[i])."""
    from unet_dc_segmentation_amd.device_data import DeviceTrainLoader
    ids = [3 * i + 1000 for i in range(N_SMALL)]
    shard = DeviceTrainLoader(small_cache, 36, seed=11, ids=ids, sigma=SMALL_SIGMA, alpha=SMALL_ALPHA)
    assert _two_epochs_match_host(shard) >= 10
    whole = DeviceTrainLoader(small_cache, 36, seed=11, sigma=SMALL_SIGMA, alpha=SMALL_ALPHA)
    idx = np.arange(36)
    a, b = shard.batch(0, idx), whole.batch(0, idx)
    assert not torch.equal(a[0], b[0])


def test_train_loader_batch_does_not_depend_on_the_batch_before(small_cache):
    """_fields and _ws are reused: a batch after one with MORE elastic samples must not read that batch's fields."""
    from unet_dc_segmentation_amd.augment import draw_params
    from unet_dc_segmentation_amd.device_data import DeviceTrainLoader
    seed, epoch = 5, 1
    el = [draw_params(seed, epoch, i)["elastic"] for i in range(N_SMALL)]
    yes, no = [i for i in range(N_SMALL) if el[i]], [i for i in range(N_SMALL) if not el[i]]
    assert len(yes) >= 6 and len(no) >= 6
    before = np.array(yes[:-2] + no[:2])                             # many elastic samples: many field slots written
    this = np.array([no[2], yes[-1], no[3], yes[-2], no[4]])         # two elastic samples: slots 0 and 1
    loader = DeviceTrainLoader(small_cache, len(before), seed=seed, sigma=SMALL_SIGMA, alpha=SMALL_ALPHA)
    loader.batch(epoch, before)
    got = loader.batch(epoch, this)
    fresh = DeviceTrainLoader(small_cache, len(before), seed=seed, sigma=SMALL_SIGMA, alpha=SMALL_ALPHA).batch(epoch, this)
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    assert _assert_batch_matches_host(loader, _host(small_cache), epoch, this, got) == 2


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
