"""GPU: native-resolution crops (csrc/crop.hip, unet_dc_segmentation_amd/device_data.py, train_DC_focal.py --crop) against the
numpy statement of the rule (utils/crops.py), against the existing augmentation gather on a cache of the same windows, and
end to end through main().  Fixtures and the refused calls: tests/crops_ref.py."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import crops_ref as cr
from tests import image_edge_fixtures as fx
from tests.image_canaries import Canaried, canaried_like
from utils import crops

pytestmark = pytest.mark.gpu

S = cr.S
BATCH = 33                          # one more than AUG_MAX_BATCH: every full batch takes two launches


def _flat(imgs, masks):
    """The images / masks back to back in two canaried device buffers + their byte offsets."""
    ci = canaried_like(np.concatenate([i.reshape(-1) for i in imgs]))
    cm = canaried_like(np.concatenate([m.reshape(-1) for m in masks]))
    pix = np.concatenate([[0], np.cumsum([m.size for m in masks])]).astype(np.int64)
    return ci, cm, [int(v) * imgs[0].shape[2] for v in pix[:-1]], [int(v) for v in pix[:-1]]


def _gather(imgs, masks, recs, fields=None):
    """unetdc_crop_gather on `recs` (crops_ref records) with canaried caches and outputs -> numpy (images, masks)."""
    from unet_dc_segmentation_amd.crops import crop_gather, pack_crops
    ci, cm, ioff, moff = _flat(imgs, masks)
    c, n = imgs[0].shape[2], len(recs)
    rec, seeds = pack_crops([r["params"] for r in recs], [ioff[r["img"]] for r in recs], [moff[r["img"]] for r in recs],
                            [masks[r["img"]].shape for r in recs], [(r["y0"], r["x0"]) for r in recs],
                            [crops.image_max(imgs[r["img"]]) for r in recs])
    oi, om = Canaried(n * c * S * S * 4), Canaried(n * S * S * 4)
    crop_gather(ci.u8, cm.u8, c, S, rec, fields, out_img=oi.view(torch.float32, n, c, S, S),
                out_mask=om.view(torch.float32, n, 1, S, S))
    torch.cuda.synchronize()
    for v, what in ((oi, "cropped images"), (om, "cropped masks"), (ci, "image cache"), (cm, "mask cache")):
        v.check(what)
    assert np.array_equal(ci.numpy(np.uint8, -1), np.concatenate([i.reshape(-1) for i in imgs]))      # the caches are only read
    assert np.array_equal(cm.numpy(np.uint8, -1), np.concatenate([m.reshape(-1) for m in masks]))
    return oi.numpy(np.float32, n, c, S, S), om.numpy(np.float32, n, 1, S, S), rec, seeds


@pytest.fixture(scope="module")
def expected():
    """{channels: (images, masks, records, crop_gather_numpy of all 192 records)}: computed once, never changed."""
    out = {}
    for c in (1, 3):
        imgs, masks = cr.images(c, bright=(c == 3), seed=40 + c)
        recs = cr.records(seed=50 + c)
        out[c] = (imgs, masks, recs, crops.crop_gather_numpy(imgs, masks, recs, S))
    return out


@pytest.mark.parametrize("c", [1, 3])
def test_gather_without_elastic_is_bit_equal_to_numpy(expected, c):
    """Every image of crops_ref.SHAPES at its end origins, every k, both flips, brightness / contrast, in batches of 33."""
    imgs, masks, recs, (ei, em) = expected[c]
    assert len(recs) == 192
    for b0 in range(0, len(recs), BATCH):
        oi, om, rec, seeds = _gather(imgs, masks, recs[b0:b0 + BATCH])
        assert len(seeds) == 0 and (rec["field"] == -1).all()
        for j in range(len(oi)):
            assert np.array_equal(oi[j].view(np.uint32), ei[b0 + j].view(np.uint32)), (c, recs[b0 + j])
            assert np.array_equal(om[j], em[b0 + j]), (c, recs[b0 + j])


@pytest.mark.parametrize("elastic", [False, True])
def test_gather_is_bit_equal_to_augment_gather_on_the_windows(expected, elastic):
    """Images at least as large as the crop: unetdc_crop_gather == unetdc_augment_gather on a float32 cache that holds the
    same windows (the new path is the old augmentation at a new scale).  With elastic both read the same device fields and
    do the same float32 operations in the same order."""
    from unet_dc_segmentation_amd.augment import augment_gather, elastic_fields, pack_params
    imgs, masks, recs, _ = expected[3]
    recs = [dict(r) for r in recs if min(masks[r["img"]].shape) >= S][::4][:BATCH]
    assert len(recs) == BATCH and {r["img"] for r in recs} == {0, 1, 4}
    if elastic:
        for j, r in enumerate(recs):
            r["params"] = dict(r["params"], elastic=j % 5 != 2, field_seed=77 + j)
    wins = [crops.window(imgs[r["img"]], masks[r["img"]], r["y0"], r["x0"], S) for r in recs]
    # np.stack keeps the stride order of its transposed inputs; the cache must be contiguous [M, C, S, S]
    cache_img = torch.from_numpy(np.ascontiguousarray(np.stack([w.transpose(2, 0, 1) for w, _ in wins]))).cuda()
    cache_mask = torch.from_numpy(np.stack([np.ascontiguousarray(m) for _, m in wins])).cuda()
    arec, seeds = pack_params([r["params"] for r in recs], list(range(len(recs))), [crops.image_max(imgs[r["img"]]) for r in recs])
    fields = elastic_fields(seeds, S, S, 3.0, 40.0) if elastic else None
    assert (len(seeds) > 20) == elastic
    wi, wm = augment_gather(cache_img, cache_mask, arec, fields)
    oi, om, rec, seeds2 = _gather(imgs, masks, recs, fields)
    assert np.array_equal(seeds, seeds2) and np.array_equal(rec["field"], arec["field"]) and np.array_equal(rec["beta_max"], arec["beta_max"])
    assert np.array_equal(oi.view(np.uint32), wi.cpu().numpy().view(np.uint32))
    assert np.array_equal(om, wm.cpu().numpy())


def _assert_elastic_sample(oi, om, ei, em, dx, dy, what):
    """The tolerances tests/test_gpu_augment.py applies to the existing gather: image <= 5e-5, mask equal outside the near-tie
    set, which may cover at most 2 %."""
    assert np.abs(oi - ei).max() <= 5e-5, (what, np.abs(oi - ei).max())
    tie = fx.near_tie(dx, dy)
    assert tie.mean() <= fx.NEAR_TIE_CAP, (what, tie.mean())
    diff = om[0] != em[0]
    assert not (diff & ~tie).any(), (what, int(diff.sum()), int(tie.sum()))


def test_gather_with_elastic_matches_numpy(expected):
    """All five images (folded ones included), 33 samples, 29 of them elastic, displacements of several pixels: against
    crop_gather_numpy (scipy.ndimage.map_coordinates, mode="reflect" at the WINDOW's border) on the device's own fields."""
    from unet_dc_segmentation_amd.augment import elastic_fields
    imgs, masks, recs, _ = expected[3]
    recs = [dict(r) for r in recs[::5]][:BATCH]
    assert len(recs) == BATCH and {r["img"] for r in recs} == {0, 1, 2, 3, 4}
    plain = (3, 11, 20, 32)
    for j, r in enumerate(recs):
        r["params"] = dict(r["params"], elastic=j not in plain, field_seed=int(fx.field_seeds(BATCH)[j]))
    seeds = np.array([r["params"]["field_seed"] for r in recs if r["params"]["elastic"]], dtype=np.uint32)
    fields = elastic_fields(seeds, S, S, 3.0, 40.0)
    fh = fields.cpu().numpy().astype(np.float64)
    assert np.abs(fh).max() > 2.0
    oi, om, rec, seeds2 = _gather(imgs, masks, recs, fields)
    assert np.array_equal(seeds, seeds2)
    assert set(np.unique(om).tolist()) <= {0.0, 1.0}
    host_fields = [(fh[rec[j]["field"], 0], fh[rec[j]["field"], 1]) if rec[j]["field"] >= 0 else None for j in range(BATCH)]
    ei, em = crops.crop_gather_numpy(imgs, masks, recs, S, host_fields)
    slot = 0
    for j, r in enumerate(recs):
        if j in plain:
            assert rec[j]["field"] == -1
            assert np.array_equal(oi[j].view(np.uint32), ei[j].view(np.uint32)) and np.array_equal(om[j], em[j]), r
            continue
        assert rec[j]["field"] == slot
        _assert_elastic_sample(oi[j], om[j], ei[j], em[j], *host_fields[j], (j, r))
        slot += 1
    assert slot == len(seeds) == BATCH - len(plain)


@pytest.mark.parametrize("name", sorted(cr.REFUSED))
def test_refused_calls_return_einval_and_launch_nothing(name):
    from unet_dc_segmentation_amd import _lib
    imgs, masks = cr.images(3)
    ci, cm = canaried_like(imgs[0]), canaried_like(masks[0])
    oi, om = Canaried(3 * S * S * 4), Canaried(S * S * 4)
    rc = cr.refused_call(_lib.load(), name, dict(images=ci.ptr, masks=cm.ptr, out_img=oi.ptr, out_mask=om.ptr))
    torch.cuda.synchronize()
    assert rc == -1, name                                             # UNETDC_EINVAL
    assert oi.untouched() and om.untouched()
    for v in (oi, om, ci, cm):
        v.check(name)


# ---- cache and loaders on PNG files: six pairs of 48 x 80 and 30 x 44 -------------------------------------------------------------
N_PAIRS, RADIUS = 6, 7
SIGMA, ALPHA = 3.0, 40.0            # displacements of pixels on a 32 x 32 window (the training defaults move nothing there)


def _write_pairs(d):
    import bench
    ind, md = d / "images", d / "masks"
    ind.mkdir()
    md.mkdir()
    names = [f"p_{i}.png" for i in range(N_PAIRS)]
    for i, name in enumerate(names):
        h, w = (48, 80) if i % 2 == 0 else (30, 44)
        img = bench.synthetic_micrograph(900 + i, h=h, w=w, discs=3)
        mask = img[..., 0] > 110
        assert 0.05 < mask.mean() < 0.95, (name, mask.mean())         # every split has droplets and background
        Image.fromarray(img).save(ind / name)
        Image.fromarray(mask.astype(np.uint8) * 255).save(md / name)
    return str(ind), str(md), names


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    return _write_pairs(tmp_path_factory.mktemp("crops"))


@pytest.fixture(scope="module")
def cache(data_dir):
    from unet_dc_segmentation_amd.device_data import DeviceNativeCache
    return DeviceNativeCache(data_dir[0], data_dir[1], data_dir[2], RADIUS, "cuda")


@pytest.fixture(scope="module")
def host(cache):
    """The cache's images and masks as numpy lists (one read-back)."""
    return [cache.image(i).cpu().numpy() for i in range(len(cache))], [cache.mask(i).cpu().numpy() for i in range(len(cache))]


def test_native_cache_holds_the_corrected_images_at_their_own_size(data_dir, cache, host):
    from utils.data_loader import rolling_ball_correction_rgb
    ind, md, names = data_dir
    assert len(cache) == N_PAIRS and cache.sizes == [(48, 80), (30, 44)] * 3
    assert cache.images.numel() == 3 * cache.masks.numel() == 3 * 3 * (48 * 80 + 30 * 44)
    for i, name in enumerate(names):
        img = np.array(Image.open(os.path.join(ind, name)).convert("RGB"))
        mask = (np.array(Image.open(os.path.join(md, name)).convert("L")) > 0).astype(np.uint8)
        want = rolling_ball_correction_rgb(img, RADIUS)
        assert np.array_equal(host[0][i], want) and np.array_equal(host[1][i], mask), name
        assert cache.img_max[i] == crops.image_max(want)
        assert cache.img_off[i] == 3 * cache.mask_off[i] == 3 * sum(h * w for h, w in cache.sizes[:i])


def _epoch(loader):
    """One epoch of the loader as host arrays: (images [n, 3, S, S], masks [n, 1, S, S], names)."""
    batches = list(loader)
    assert len(batches) == len(loader)
    for b in batches:
        assert b[0].shape[1:] == (3, S, S) and b[1].shape[1:] == (1, S, S) and len(b[3]) == len(b[0]) == len(b[2][0]) == len(b[2][1])
    return (torch.cat([b[0] for b in batches]).cpu().numpy(), torch.cat([b[1] for b in batches]).cpu().numpy(),
            [n for b in batches for n in b[3]], torch.cat([torch.stack(b[2], 1) for b in batches]).tolist())


def test_train_loader_is_deterministic_and_independent_of_the_batch_size(cache, host):
    from unet_dc_segmentation_amd.device_data import DeviceCropTrainLoader
    R, ids = 3, [10, 11, 12, 13, 14, 15]
    mk = lambda batch: DeviceCropTrainLoader(cache, batch, S, seed=5, ids=ids, crops_per_image=R, sigma=SIGMA, alpha=ALPHA)  # noqa: E731
    a, b, c = mk(3), mk(3), mk(8)
    assert len(a) == 6 and len(c) == 3 and a.samples == N_PAIRS * R
    ea, eb, ec = [_epoch(a), _epoch(a)], [_epoch(b), _epoch(b)], [_epoch(c), _epoch(c)]
    for e in range(2):
        for other in (eb[e], ec[e]):
            assert np.array_equal(ea[e][0].view(np.uint32), other[0].view(np.uint32)) and np.array_equal(ea[e][1], other[1])
            assert ea[e][2] == other[2] and ea[e][3] == other[3]
        assert len(ea[e][2]) == N_PAIRS * R and sorted(ea[e][2]) == sorted(cache.names * R)
        assert set(np.unique(ea[e][1]).tolist()) <= {0.0, 1.0} and ea[e][0].min() >= 0 and ea[e][0].max() <= 1
    assert not np.array_equal(ea[0][0], ea[1][0])
    # every sample against the host statement of its own draw: window from draw_crop, augmentation from draw_params, both
    # keyed by the sample number q = ids[i] * R + rep of the whole split
    from unet_dc_segmentation_amd.augment import draw_params, elastic_fields
    nel = 0
    for e in range(2):
        perm = np.random.default_rng([5, e]).permutation(N_PAIRS * R)
        recs, fields = [], []
        for j in perm:
            i, q = int(j) // R, ids[int(j) // R] * R + int(j) % R
            p = draw_params(5, e, q)
            y0, x0 = crops.draw_crop(5, e, q, *cache.sizes[i], S)
            recs.append(dict(img=i, y0=y0, x0=x0, params=p))
            fields.append(p["field_seed"] if p["elastic"] else None)
        # the fields of the samples that draw elastic, made by the device once more from the same seeds (bitwise reproducible)
        fh = elastic_fields(np.array([f for f in fields if f is not None], dtype=np.uint32), S, S, SIGMA, ALPHA).cpu().numpy()
        slots = iter(fh.astype(np.float64))
        fields = [None if f is None else tuple(next(slots)) for f in fields]
        assert ea[e][2] == [cache.names[r["img"]] for r in recs]
        assert ea[e][3] == [list(cache.sizes[r["img"]]) for r in recs]
        wi, wm = crops.crop_gather_numpy(host[0], host[1], recs, S, fields)
        for j, r in enumerate(recs):
            if r["params"]["elastic"]:
                _assert_elastic_sample(ea[e][0][j], ea[e][1][j], wi[j], wm[j], *fields[j], (e, j, r))
                nel += 1
            else:
                assert np.array_equal(ea[e][0][j].view(np.uint32), wi[j].view(np.uint32)) and np.array_equal(ea[e][1][j], wm[j]), (e, j, r)
    assert nel >= 4


def test_eval_loader_returns_every_image_at_its_eval_plan(cache, host):
    from unet_dc_segmentation_amd.device_data import DeviceCropEvalLoader
    want = [(i, y0, x0) for i, (h, w) in enumerate(cache.sizes) for y0, x0 in crops.eval_plan(h, w, S)]
    assert len(want) == 3 * (2 * 3 + 1 * 2)                           # 48 x 80: 2 x 3 windows; 30 x 44: 1 x 2
    for batch in (4, 32):
        loader = DeviceCropEvalLoader(cache, batch, S)
        assert loader.windows == want and len(loader) == -(-len(want) // batch) and loader.dataset is cache
        gi, gm, names, sizes = _epoch(loader)
        assert names == [cache.names[i] for i, _, _ in want] and sizes == [list(cache.sizes[i]) for i, _, _ in want]
        for j, (i, y0, x0) in enumerate(want):
            win, mwin = crops.window(host[0][i], host[1][i], y0, x0, S)
            assert np.array_equal(gi[j].view(np.uint32), win.transpose(2, 0, 1).view(np.uint32)), (i, y0, x0)
            assert np.array_equal(gm[j, 0], mwin.astype(np.float32)), (i, y0, x0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_crop_trains_end_to_end(data_dir, tmp_path, monkeypatch, capsys, dtype):
    """--crop 32 through main() in both compute types.  bf16: the same step on the small bf16 routes (a 2 x 2 bottleneck, batches
    of 4 on four training images); val_dice > 0 stays an fp32-only assertion (two epochs from a random start in bf16 is not a
    measured quantity)."""
    import train_DC_focal
    from unet_dc_segmentation_amd import device_data
    served = []
    batch = device_data.DeviceCropTrainLoader.batch
    monkeypatch.setattr(device_data.DeviceCropTrainLoader, "batch",
                        lambda self, epoch, js: (served.append((epoch, len(js), len(self.dataset))), batch(self, epoch, js))[1])
    h = train_DC_focal.main(["--image_dir", data_dir[0], "--mask_dir", data_dir[1], "--ckpt_path", str(tmp_path / "ck.pth"),
                             "--device_data", "--crop", "32", "--crops_per_image", "2", "--batch", "4", "--epochs", "2",
                             "--patience", "5", "--calibrate_thresh", "10"] + (["--dtype", "bf16"] if dtype == "bf16" else []))
    assert len(h) == 2
    for rec in h:
        assert all(math.isfinite(rec[k]) for k in ("train_loss", "val_loss", "train_dice", "val_dice"))
    n_train = served[0][2]
    assert n_train == N_PAIRS - 2                                     # 6 files: 1 test, 1 validation, 4 training images
    for e in range(2):
        assert sum(n for ep, n, _ in served if ep == e) == 2 * n_train
    assert h.test is not None and math.isfinite(h.test["test_loss"])
    assert os.path.exists(tmp_path / "ck.pth")
    if dtype == "f32":
        assert max(rec["val_dice"] for rec in h) > 0                  # every split has droplets
    c = h.calibration
    assert c is not None and c["K"] == 10 and 0 <= c["best_dice_threshold"] < 1 and int(np.asarray(c["hist"]).sum()) > 0
    out = capsys.readouterr().out
    assert "--img_size 512 is not used" in out and "Threshold calibration" in out
