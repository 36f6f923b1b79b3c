"""CPU: the numpy restatement of the device augmentation (tests/augment_ref.py) against TrainAugment, the host-side parameter
draws of unet_dc_segmentation_amd.augment, the noise hash, the new C-ABI entry points' argument checks, and the
--device_data flag's refusal on a CPU device."""
import ctypes
import itertools

import numpy as np
import pytest
from scipy import ndimage

from tests import augment_ref as ref
from utils.data_loader import TrainAugment


class ScriptedRng:
    """Stands in for TrainAugment's generator: random() / integers() / uniform() return scripted values, random(shape)
    returns scripted arrays (the elastic noise)."""

    def __init__(self, values, arrays=()):
        self.values, self.arrays = list(values), list(arrays)

    def random(self, size=None):
        return self.arrays.pop(0) if size is not None else self.values.pop(0)

    def integers(self, lo, hi):
        return self.values.pop(0)

    def uniform(self, lo, hi):
        return self.values.pop(0)


def run_train_augment(img, mask, p, arrays=()):
    vals = [0.0 if p["hflip"] else 0.9, 0.0 if p["vflip"] else 0.9, 0.0 if p["k"] else 0.9]
    if p["k"]:
        vals.append(p["k"])
    vals.append(0.0 if p["bc"] else 0.9)
    if p["bc"]:
        vals += [p["alpha"] - 1.0, p["beta"]]
    vals.append(0.0 if p["elastic"] else 0.9)
    t = TrainAugment(0)
    rng = ScriptedRng(vals, arrays)
    t._generator = lambda: rng
    out = t(img, mask)
    assert not rng.values and not rng.arrays
    return out


def sample(h=24, w=24, seed=0):
    r = np.random.default_rng(seed)
    img = (r.integers(0, 256, (h, w, 3)) / 255.0).astype(np.float32)
    return img, (r.random((h, w)) < 0.3).astype(np.uint8)


def params(hflip, vflip, k, bc, elastic=False, alpha=1.13, beta=-0.07):
    return dict(hflip=hflip, vflip=vflip, k=k, bc=bc, alpha=alpha if bc else 1.0, beta=beta if bc else 0.0,
                elastic=elastic, field_seed=0)


@pytest.mark.parametrize("hflip,vflip,k,bc", list(itertools.product([0, 1], [0, 1], [0, 1, 2, 3], [0, 1])))
def test_restatement_matches_train_augment(hflip, vflip, k, bc):
    img, mask = sample(20, 20)
    p = params(bool(hflip), bool(vflip), k, bool(bc))
    ei, em = run_train_augment(img, mask, p)
    gi, gm = ref.augment_with_params(img, mask, p)
    assert ei.dtype == gi.dtype == np.float32 and np.array_equal(ei.view(np.uint32), gi.view(np.uint32))
    assert np.array_equal(em, gm)


@pytest.mark.parametrize("k,bc", [(0, False), (1, True), (3, False)])
def test_restatement_matches_train_augment_elastic(k, bc):
    img, mask = sample(32, 32, seed=3)
    r = np.random.default_rng(5)
    u1, u2 = r.random((32, 32)), r.random((32, 32))
    p = params(True, False, k, bc, elastic=True)
    ei, em = run_train_augment(img, mask, p, arrays=[u1, u2])
    dx = ndimage.gaussian_filter(u1 * 2 - 1, 50.0, mode="constant") * 1.0
    dy = ndimage.gaussian_filter(u2 * 2 - 1, 50.0, mode="constant") * 1.0
    gi, gm = ref.augment_with_params(img, mask, p, dx, dy)
    assert np.array_equal(ei.view(np.uint32), gi.view(np.uint32)) and np.array_equal(em, gm)


def test_param_draws_deterministic_and_independent_of_batching():
    from unet_dc_segmentation_amd.augment import draw_params
    a = [draw_params(42, 3, i) for i in range(40)]
    assert a == [draw_params(42, 3, i) for i in range(40)]
    assert a != [draw_params(42, 4, i) for i in range(40)] and a != [draw_params(43, 3, i) for i in range(40)]
    # a sample's draw depends on (seed, epoch, index) only: the same whatever batch or rank shard it is visited in
    for bs, world in [(1, 1), (8, 1), (5, 2), (8, 4)]:
        got = {}
        for rank in range(world):
            shard = list(range(rank, 40, world))
            for b0 in range(0, len(shard), bs):
                for i in shard[b0:b0 + bs]:
                    got[i] = draw_params(42, 3, i)
        assert [got[i] for i in range(40)] == a


def test_param_draw_frequencies():
    from unet_dc_segmentation_amd.augment import draw_params
    n = 20000
    ps = [draw_params(7, 0, i) for i in range(n)]

    def near(count, p):
        return abs(count - n * p) <= 5 * np.sqrt(n * p * (1 - p))
    assert near(sum(p["hflip"] for p in ps), 0.5)
    assert near(sum(p["vflip"] for p in ps), 0.2)
    rot = [p["k"] for p in ps if p["k"]]
    assert near(len(rot), 0.5)
    assert near(sum(p["bc"] for p in ps), 0.2)
    assert near(sum(p["elastic"] for p in ps), 0.3)
    m = len(rot)
    for k in (1, 2, 3):
        assert abs(rot.count(k) - m / 3) <= 5 * np.sqrt(m * (1 / 3) * (2 / 3))
    bc = [p for p in ps if p["bc"]]
    assert all(0.8 <= p["alpha"] <= 1.2 and -0.2 <= p["beta"] <= 0.2 for p in bc)
    assert len({p["field_seed"] for p in ps if p["elastic"]}) > 0.99 * sum(p["elastic"] for p in ps)


def test_pack_params_layout():
    from unet_dc_segmentation_amd import augment
    ps = [params(True, False, 1, True, alpha=1.1, beta=0.1), params(False, True, 0, False, elastic=True),
          params(False, False, 2, False, elastic=True)]
    ps[1]["field_seed"], ps[2]["field_seed"] = 11, 2 ** 32 - 1
    rec, seeds = augment.pack_params(ps, [4, 0, 2], [0.5, 1.0, 0.25])
    assert augment.PARAMS_DTYPE.itemsize == 32
    assert list(rec["src"]) == [4, 0, 2] and list(rec["field"]) == [-1, 0, 1] and list(rec["k"]) == [1, 0, 2]
    assert list(rec["flags"]) == [augment.HFLIP | augment.BC, augment.VFLIP, 0]
    assert rec["alpha"][0] == np.float32(1.1) and rec["beta_max"][0] == np.float32(0.1 * 0.5)
    assert seeds.dtype == np.uint32 and list(seeds) == [11, 2 ** 32 - 1]


def test_noise_hash_range_and_mean():
    a = np.concatenate([ref.noise(s, c, 64, 96).ravel() for s in (0, 1, 2 ** 31 + 5) for c in (0, 1)])
    assert a.dtype == np.float32 and a.min() >= -1.0 and a.max() < 1.0
    assert abs(a.mean()) <= 5 * np.sqrt(1 / 3 / a.size)
    assert not np.array_equal(ref.noise(1, 0, 8, 8), ref.noise(1, 1, 8, 8))
    assert not np.array_equal(ref.noise(1, 0, 8, 8), ref.noise(2, 0, 8, 8))
    # 24-bit uniforms: every value is a multiple of 2^-23
    assert np.array_equal(np.round(a * 2.0 ** 23), a * 2.0 ** 23)


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_abi_entry_points_validate_without_gpu(lib):
    from unet_dc_segmentation_amd import _lib, augment
    for name in ("unetdc_elastic_fields_workspace", "unetdc_elastic_fields", "unetdc_augment_gather"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.unetdc_version() == 2
    ws = lib.unetdc_elastic_fields_workspace(8, 512, 512, 50.0)
    assert ws >= 4 * 8 * 2 * 512 * 512 + 4 * 401
    assert lib.unetdc_elastic_fields_workspace(1, 512, 512, -1.0) < 0
    seeds = (ctypes.c_uint32 * 2)(1, 2)
    fake = ctypes.c_void_p(0x1000)              # never dereferenced: validation fails before any HIP call
    rc = lib.unetdc_elastic_fields(seeds, 2, 2048, 2048, 50.0, 1.0, fake, fake, 1 << 40, None)
    assert rc == -1 and b"geometry" in lib.unetdc_last_error()
    rc = lib.unetdc_elastic_fields(seeds, 2, 64, 64, 300.0, 1.0, fake, fake, 1 << 40, None)
    assert rc == -1 and b"sigma" in lib.unetdc_last_error()
    rc = lib.unetdc_elastic_fields(seeds, 2, 64, 64, 5.0, 1.0, None, fake, 1 << 40, None)
    assert rc == -1 and b"null" in lib.unetdc_last_error()
    rc = lib.unetdc_elastic_fields(seeds, 2, 64, 64, 5.0, 1.0, fake, fake, 16, None)
    assert rc == -3 and b"workspace" in lib.unetdc_last_error()

    def gather(rec, h=8, w=8, ncache=3, nfields=0, fields=None):
        rec = np.ascontiguousarray(rec, dtype=augment.PARAMS_DTYPE)
        return lib.unetdc_augment_gather(fake, fake, ncache, 3, h, w, rec.ctypes.data, len(rec), fields, nfields, fake,
                                         fake, None)
    rec = np.zeros(2, dtype=augment.PARAMS_DTYPE)
    rec["field"] = -1
    bad = rec.copy(); bad[1]["src"] = 3
    assert gather(bad) == -1 and b"source index" in lib.unetdc_last_error()
    bad = rec.copy(); bad[0]["k"] = 1
    assert gather(bad, h=8, w=6) == -1 and b"square" in lib.unetdc_last_error()
    bad = rec.copy(); bad[0]["k"] = 4
    assert gather(bad) == -1 and b"k = 4" in lib.unetdc_last_error()
    bad = rec.copy(); bad[0]["field"] = 0
    assert gather(bad) == -1 and b"field slot" in lib.unetdc_last_error()
    assert gather(bad, nfields=1) == -1 and b"fields is null" in lib.unetdc_last_error()
    bad = rec.copy(); bad[0]["flags"] = 8
    assert gather(bad) == -1 and b"flags" in lib.unetdc_last_error()
    assert lib.unetdc_augment_gather(fake, fake, 0, 3, 8, 8, rec.ctypes.data, 2, None, 0, fake, fake, None) == -1


def test_device_data_flag_refuses_cpu(tmp_path):
    import train_DC_focal
    with pytest.raises(SystemExit) as e:
        train_DC_focal.main(["--device_data", "--device", "cpu", "--image_dir", str(tmp_path), "--mask_dir",
                             str(tmp_path), "--epochs", "1"])
    assert "--device_data" in str(e.value) and "cpu" in str(e.value)
