"""GPU: scale jitter and foreground-aware windows (csrc/crop.hip:crop_gather_scaled_kernel, device_data.py, train_DC_focal.py
--crop_scale / --crop_fg) against the numpy statement of the rule (utils/crops.py), against unetdc_crop_gather at T = S, and
end to end through main().  Fixtures and the refused calls: tests/crops_ref.py, tests/crop_scale_ref.py."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import crop_scale_ref as sr
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


class Caches:
    """The canaried device caches of one list of images, made once and checked after every gather."""

    def __init__(self, imgs, masks):
        self.imgs, self.masks = imgs, masks
        self.ci, self.cm, self.ioff, self.moff = _flat(imgs, masks)
        self.flat_i = np.concatenate([i.reshape(-1) for i in imgs])
        self.flat_m = np.concatenate([m.reshape(-1) for m in masks])

    def gather(self, recs, fields=None, s=S, scaled=True):
        """unetdc_crop_gather_scaled (or unetdc_crop_gather) on `recs` with canaried outputs -> numpy (images, masks, records)."""
        from unet_dc_segmentation_amd.crops import crop_gather, crop_gather_scaled, pack_crops, pack_crops_scaled
        imgs, masks = self.imgs, self.masks
        c, n = imgs[0].shape[2], len(recs)
        args = ([r["params"] for r in recs], [self.ioff[r["img"]] for r in recs], [self.moff[r["img"]] for r in recs],
                [masks[r["img"]].shape for r in recs], [(r["y0"], r["x0"]) for r in recs],
                [crops.image_max(imgs[r["img"]]) for r in recs])
        rec, _ = pack_crops_scaled(*args, [r["T"] for r in recs]) if scaled else pack_crops(*args)
        oi, om = Canaried(n * c * s * s * 4), Canaried(n * s * s * 4)
        (crop_gather_scaled if scaled else crop_gather)(self.ci.u8, self.cm.u8, c, s, rec, fields,
                                                        out_img=oi.view(torch.float32, n, c, s, s),
                                                        out_mask=om.view(torch.float32, n, 1, s, s))
        torch.cuda.synchronize()
        for v, what in ((oi, "cropped images"), (om, "cropped masks"), (self.ci, "image cache"), (self.cm, "mask cache")):
            v.check(what)
        assert np.array_equal(self.ci.numpy(np.uint8, -1), self.flat_i)            # the caches are only read
        assert np.array_equal(self.cm.numpy(np.uint8, -1), self.flat_m)
        return oi.numpy(np.float32, n, c, s, s), om.numpy(np.float32, n, 1, s, s), rec


@pytest.fixture(scope="module")
def expected():
    """{channels: (Caches, records, crop_gather_scaled_numpy of all 1072 records)}: computed once, never changed."""
    out = {}
    for c in (1, 3):
        imgs, masks = cr.images(c, bright=(c == 3), seed=40 + c)
        recs = sr.records(seed=50 + c)
        out[c] = (Caches(imgs, masks), recs, crops.crop_gather_scaled_numpy(imgs, masks, recs, S))
    return out


@pytest.mark.parametrize("c", [1, 3])
def test_scaled_gather_without_elastic_is_bit_equal_to_numpy(expected, c):
    """Every image of crops_ref.SHAPES at its end origins for each T of 16, 31, 32, 33, 47, 64, every k, both flips, brightness
    / contrast on half, in batches of 33."""
    caches, recs, (ei, em) = expected[c]
    assert len(recs) == 67 * 16 and {r["T"] for r in recs} == set(sr.TS)
    for b0 in range(0, len(recs), BATCH):
        oi, om, rec = caches.gather(recs[b0:b0 + BATCH])
        assert (rec["field"] == -1).all()
        for j in range(len(oi)):
            assert np.array_equal(oi[j].view(np.uint32), ei[b0 + j].view(np.uint32)), (c, recs[b0 + j])
            assert np.array_equal(om[j], em[b0 + j]), (c, recs[b0 + j])


def test_scaled_gather_at_the_smallest_size():
    """S = 16, the kernel's smallest: one block per sample; T = 8, 16, 32 on every shape at its end origins."""
    s = 16
    imgs, masks = cr.images(3, bright=True, seed=61)
    recs = sr.records(seed=62, s=s, ts=[8, 16, 32])[::3]
    assert len(recs) > 150 and {r["T"] for r in recs} == {8, 16, 32} and {r["img"] for r in recs} == set(range(len(cr.SHAPES)))
    caches = Caches(imgs, masks)
    ei, em = crops.crop_gather_scaled_numpy(imgs, masks, recs, s)
    for b0 in range(0, len(recs), 2 * BATCH):
        oi, om, _ = caches.gather(recs[b0:b0 + 2 * BATCH], s=s)
        for j in range(len(oi)):
            assert np.array_equal(oi[j].view(np.uint32), ei[b0 + j].view(np.uint32)), recs[b0 + j]
            assert np.array_equal(om[j], em[b0 + j]), recs[b0 + j]


@pytest.mark.parametrize("elastic", [False, True])
def test_records_with_t_equal_s_are_bit_equal_to_crop_gather(expected, elastic):
    """All five images (folded ones included): unetdc_crop_gather_scaled with t = S == unetdc_crop_gather, both reading the same
    device fields."""
    from unet_dc_segmentation_amd.augment import elastic_fields
    caches = expected[3][0]
    recs = [dict(r, T=S) for r in cr.records(seed=53)[::5]][:BATCH]
    assert len(recs) == BATCH and {r["img"] for r in recs} == {0, 1, 2, 3, 4}
    fields = None
    if elastic:
        for j, r in enumerate(recs):
            r["params"] = dict(r["params"], elastic=j % 5 != 2, field_seed=77 + j)
        seeds = np.array([r["params"]["field_seed"] for r in recs if r["params"]["elastic"]], dtype=np.uint32)
        assert len(seeds) > 20
        fields = elastic_fields(seeds, S, S, 3.0, 40.0)
    wi, wm, wrec = caches.gather(recs, fields, scaled=False)
    oi, om, rec = caches.gather(recs, fields)
    assert np.array_equal(rec["field"], wrec["field"]) and (rec["t"] == S).all() and ((rec["field"] >= 0).sum() > 20) == elastic
    assert np.array_equal(oi.view(np.uint32), wi.view(np.uint32))
    assert np.array_equal(om, wm)


def _assert_elastic_sample(oi, om, ei, em, dx, dy, what):
    """The tolerances tests/test_gpu_crops.py applies: image <= 5e-5, mask equal outside the near-tie set, which may cover at
    most fx.NEAR_TIE_CAP."""
    assert np.abs(oi - ei).max() <= 5e-5, (what, np.abs(oi - ei).max())
    tie = fx.near_tie(dx, dy)
    assert tie.mean() <= fx.NEAR_TIE_CAP, (what, tie.mean())
    diff = om[0] != em[0]
    assert not (diff & ~tie).any(), (what, int(diff.sum()), int(tie.sum()))


def test_scaled_gather_with_elastic_matches_numpy(expected):
    """T != S on all five images, 33 samples, 29 of them elastic, the seeds, sigma and alpha of
    tests/test_gpu_crops.py::test_gather_with_elastic_matches_numpy: against crop_gather_scaled_numpy (map_coordinates on the
    scaled lattice, reflected at the window's border) on the device's own fields."""
    from unet_dc_segmentation_amd.augment import elastic_fields
    caches, recs, _ = expected[3]
    recs = [dict(r) for r in recs if r["T"] != S][::27][:BATCH]
    assert len(recs) == BATCH and {r["img"] for r in recs} == {0, 1, 2, 3, 4} and {r["T"] for r in recs} == set(sr.TS) - {S}
    plain = (3, 11, 20, 32)
    for j, r in enumerate(recs):
        r["params"] = dict(r["params"], elastic=j not in plain, field_seed=int(fx.field_seeds(BATCH)[j]))
    seeds = np.array([r["params"]["field_seed"] for r in recs if r["params"]["elastic"]], dtype=np.uint32)
    fields = elastic_fields(seeds, S, S, 3.0, 40.0)
    fh = fields.cpu().numpy().astype(np.float64)
    assert np.abs(fh).max() > 2.0
    oi, om, rec = caches.gather(recs, fields)
    assert set(np.unique(om).tolist()) <= {0.0, 1.0}
    host_fields = [(fh[rec[j]["field"], 0], fh[rec[j]["field"], 1]) if rec[j]["field"] >= 0 else None for j in range(BATCH)]
    ei, em = crops.crop_gather_scaled_numpy(caches.imgs, caches.masks, recs, S, host_fields)
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


@pytest.mark.parametrize("name", sorted(sr.REFUSED))
def test_refused_scaled_calls_return_einval_and_launch_nothing(name):
    from unet_dc_segmentation_amd import _lib
    imgs, masks = cr.images(3)
    ci, cm = canaried_like(imgs[0]), canaried_like(masks[0])
    oi, om = Canaried(3 * S * S * 4), Canaried(S * S * 4)
    rc = sr.refused_call(_lib.load(), name, dict(images=ci.ptr, masks=cm.ptr, out_img=oi.ptr, out_mask=om.ptr))
    torch.cuda.synchronize()
    assert rc == -1, name                                             # UNETDC_EINVAL
    assert oi.untouched() and om.untouched()
    for v in (oi, om, ci, cm):
        v.check(name)


def test_records_of_the_other_type_are_refused_by_the_wrapper(expected):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.crops import CROP_DTYPE, CROP_SCALED_DTYPE, crop_gather, crop_gather_scaled
    caches = expected[3][0]
    with pytest.raises(_lib.UnetdcError, match="records of another type"):
        crop_gather_scaled(caches.ci.u8, caches.cm.u8, 3, S, np.zeros(1, CROP_DTYPE))
    with pytest.raises(_lib.UnetdcError, match="records of another type"):
        crop_gather(caches.ci.u8, caches.cm.u8, 3, S, np.zeros(1, CROP_SCALED_DTYPE))


# ---- cache and loader on PNG files: six pairs of 48 x 80 and 30 x 44 (the files of tests/test_gpu_crops.py) -------------------------
N_PAIRS, RADIUS = 6, 7
SIGMA, ALPHA = 3.0, 40.0            # displacements of pixels on a 32 x 32 window (the training defaults move nothing there)
SCALE, P_FG = (0.5, 2.0), 0.5


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
    return _write_pairs(tmp_path_factory.mktemp("crop_scale"))


@pytest.fixture(scope="module")
def cache(data_dir):
    from unet_dc_segmentation_amd.device_data import DeviceNativeCache
    return DeviceNativeCache(data_dir[0], data_dir[1], data_dir[2], RADIUS, "cuda", keep_foreground=True)


@pytest.fixture(scope="module")
def host(cache):
    """The cache's images and masks as numpy lists (one read-back)."""
    return [cache.image(i).cpu().numpy() for i in range(len(cache))], [cache.mask(i).cpu().numpy() for i in range(len(cache))]


def test_native_cache_keeps_the_foreground_indices_on_request(data_dir, cache, host):
    from unet_dc_segmentation_amd.device_data import DeviceNativeCache
    assert len(cache.foreground) == N_PAIRS
    for i, fg in enumerate(cache.foreground):
        assert fg.dtype == np.int32 and np.array_equal(fg, np.flatnonzero(host[1][i])) and len(fg) > 0
    plain = DeviceNativeCache(data_dir[0], data_dir[1], data_dir[2][:2], RADIUS, "cuda")
    assert plain.foreground is None
    assert torch.equal(plain.images, cache.images[:plain.images.numel()])


def _epoch(loader):
    """One epoch of the loader as host arrays: (images [n, 3, S, S], masks [n, 1, S, S], names, sizes)."""
    batches = list(loader)
    assert len(batches) == len(loader)
    for b in batches:
        assert b[0].shape[1:] == (3, S, S) and b[1].shape[1:] == (1, S, S) and len(b[3]) == len(b[0]) == len(b[2][0]) == len(b[2][1])
    return (torch.cat([b[0] for b in batches]).cpu().numpy(), torch.cat([b[1] for b in batches]).cpu().numpy(),
            [n for b in batches for n in b[3]], torch.cat([torch.stack(b[2], 1) for b in batches]).tolist())


def test_scaled_loader_serves_the_numpy_rule_on_draw_crop_fg_records_at_any_batch_size(cache, host):
    from unet_dc_segmentation_amd.augment import draw_params, elastic_fields
    from unet_dc_segmentation_amd.device_data import DeviceCropTrainLoader
    R, ids = 3, [10, 11, 12, 13, 14, 15]
    mk = lambda batch: DeviceCropTrainLoader(cache, batch, S, seed=5, ids=ids, crops_per_image=R, sigma=SIGMA, alpha=ALPHA,  # noqa: E731
                                             scale=SCALE, p_fg=P_FG)
    a, c = mk(3), mk(8)
    assert a.scaled and len(a) == 6 and len(c) == 3 and a.samples == N_PAIRS * R
    ea, ec, counts = [], [], []
    for e in range(2):
        ea.append(_epoch(a))
        ec.append(_epoch(c))
        counts.append((a.fg_windows, c.fg_windows))
    nel, seen_t = 0, set()
    for e in range(2):
        assert np.array_equal(ea[e][0].view(np.uint32), ec[e][0].view(np.uint32)) and np.array_equal(ea[e][1], ec[e][1])
        assert ea[e][2] == ec[e][2] and ea[e][3] == ec[e][3]
        assert set(np.unique(ea[e][1]).tolist()) <= {0.0, 1.0} and ea[e][0].min() >= 0 and ea[e][0].max() <= 1
        perm = np.random.default_rng([5, e]).permutation(N_PAIRS * R)
        recs, fields, took = [], [], 0
        for j in perm:
            i, q = int(j) // R, ids[int(j) // R] * R + int(j) % R
            p = draw_params(5, e, q)
            y0, x0, T, fg = crops.draw_crop_fg_branch(5, e, q, *cache.sizes[i], S, SCALE, P_FG, cache.foreground[i])
            assert (y0, x0, T) == crops.draw_crop_fg(5, e, q, *cache.sizes[i], S, SCALE, P_FG, cache.foreground[i])
            took += fg
            seen_t.add(T)
            recs.append(dict(img=i, y0=y0, x0=x0, T=T, params=p))
            fields.append(p["field_seed"] if p["elastic"] else None)
        assert counts[e] == (took, took) and 0 < took < len(perm)
        fh = elastic_fields(np.array([f for f in fields if f is not None], dtype=np.uint32), S, S, SIGMA, ALPHA).cpu().numpy()
        slots = iter(fh.astype(np.float64))
        fields = [None if f is None else tuple(next(slots)) for f in fields]
        assert ea[e][2] == [cache.names[r["img"]] for r in recs]
        wi, wm = crops.crop_gather_scaled_numpy(host[0], host[1], recs, S, fields)
        for j, r in enumerate(recs):
            if r["params"]["elastic"]:
                _assert_elastic_sample(ea[e][0][j], ea[e][1][j], wi[j], wm[j], *fields[j], (e, j, r))
                nel += 1
            else:
                assert np.array_equal(ea[e][0][j].view(np.uint32), wi[j].view(np.uint32)) and np.array_equal(ea[e][1][j], wm[j]), (e, j, r)
    assert nel >= 4 and len(seen_t) > 10 and min(seen_t) < S < max(seen_t)


def test_foreground_alone_keeps_t_at_s_and_goes_through_the_scaled_entry_point(cache, host, monkeypatch):
    from unet_dc_segmentation_amd import crops as dcrops
    from unet_dc_segmentation_amd.device_data import DeviceCropTrainLoader
    called = []
    scaled = dcrops.crop_gather_scaled
    monkeypatch.setattr(dcrops, "crop_gather_scaled", lambda *a, **k: (called.append(a[4]["t"].tolist()), scaled(*a, **k))[1])
    loader = DeviceCropTrainLoader(cache, 4, S, seed=9, p_fg=1.0)              # (the default field moves nothing at 32 x 32)
    gi, gm, names, _ = _epoch(loader)
    assert loader.scaled and loader.scale is None and loader.fg_windows == N_PAIRS
    assert len(called) == 2 and all(t == S for ts in called for t in ts)
    assert (gm.reshape(N_PAIRS, -1).max(axis=1) == 1.0).all()          # every window holds foreground


def test_with_both_options_off_the_loader_is_the_one_built_without_them(cache, monkeypatch):
    from unet_dc_segmentation_amd import crops as dcrops
    from unet_dc_segmentation_amd.device_data import DeviceCropTrainLoader
    monkeypatch.setattr(dcrops, "crop_gather_scaled", lambda *a, **k: pytest.fail("the scaled entry point was called"))
    monkeypatch.setattr(crops, "draw_crop_fg_branch", lambda *a, **k: pytest.fail("draw_crop_fg was called"))
    kw = dict(seed=5, ids=[10, 11, 12, 13, 14, 15], crops_per_image=2, sigma=SIGMA, alpha=ALPHA)
    old, new = DeviceCropTrainLoader(cache, 5, S, **kw), DeviceCropTrainLoader(cache, 5, S, scale=None, p_fg=0.0, **kw)
    assert not new.scaled
    for e in range(2):
        a, b = _epoch(old), _epoch(new)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
        assert new.fg_windows == 0
    with pytest.raises(ValueError, match="keep_foreground"):
        from unet_dc_segmentation_amd.device_data import DeviceNativeCache
        bare = DeviceNativeCache.__new__(DeviceNativeCache)
        bare.foreground = None
        bare.names = []
        bare.device = cache.device
        DeviceCropTrainLoader(bare, 4, S, p_fg=0.5)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_scaled_crop_trains_end_to_end(data_dir, tmp_path, capsys, dtype):
    """--crop 32 --crop_scale 0.5 2 --crop_fg 0.5 through main() in both compute types, on the files and with the arguments of
    tests/test_gpu_crops.py::test_crop_trains_end_to_end."""
    import train_DC_focal
    h = train_DC_focal.main(["--image_dir", data_dir[0], "--mask_dir", data_dir[1], "--ckpt_path", str(tmp_path / "ck.pth"),
                             "--device_data", "--crop", "32", "--crop_scale", "0.5", "2", "--crop_fg", "0.5",
                             "--crops_per_image", "2", "--batch", "4", "--epochs", "2", "--patience", "5",
                             "--calibrate_thresh", "10"] + (["--dtype", "bf16"] if dtype == "bf16" else []))
    assert len(h) == 2
    for rec in h:
        assert all(math.isfinite(rec[k]) for k in ("train_loss", "val_loss", "train_dice", "val_dice"))
        assert 0 <= rec["fg_windows"] <= 8                            # 4 training images, 2 windows each
    assert sum(rec["fg_windows"] for rec in h) > 0
    assert h.test is not None and math.isfinite(h.test["test_loss"])
    assert os.path.exists(tmp_path / "ck.pth")
    assert h.calibration is not None and h.calibration["K"] == 10
    out = capsys.readouterr().out
    assert "source windows of side T in 16..64 resampled to 32 x 32" in out and "probability P = 0.5" in out
    assert out.count("Foreground-centred windows: ") == 2 and f"Foreground-centred windows: {h[0]['fg_windows']} of 8" in out
    assert "--img_size 512 is not used" in out and "Threshold calibration" in out
