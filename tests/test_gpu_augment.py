"""GPU: the augmentation kernels (csrc/augment.hip) against the numpy restatement in tests/augment_ref.py -- displacement
fields against scipy.ndimage.gaussian_filter of the restated noise, the gather bit-exact without elastic and within float32
interpolation error with it."""
import itertools

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import augment_ref as ref
from tests import image_edge_fixtures as fx
from tests.image_canaries import Canaried

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h,w,sigma,seeds", [(512, 512, 50.0, (7, 2 ** 32 - 3)), (1024, 1024, 50.0, (11,)),
                                             (96, 130, 3.0, (1, 2, 3)), (64, 64, 40.0, (5,))])
def test_fields_match_gaussian_filter_of_noise(h, w, sigma, seeds):
    from unet_dc_segmentation_amd.augment import elastic_fields
    f = elastic_fields(np.array(seeds, dtype=np.uint32), h, w, sigma, 1.0).cpu().numpy()
    assert f.shape == (len(seeds), 2, h, w)
    for i, s in enumerate(seeds):
        for c, want in enumerate(ref.fields(s, h, w, sigma, 1.0)):
            err = np.abs(f[i, c] - want).max()
            assert err <= 1e-5 * np.abs(want).max(), (s, c, err, np.abs(want).max())


def _cache(m, h, w, seed=0, c=3):
    r = np.random.default_rng(seed)
    imgs = (r.integers(0, 256, (m, c, h, w)) / 255.0).astype(np.float32)
    masks = (r.random((m, h, w)) < 0.3).astype(np.uint8)
    return imgs, masks, torch.from_numpy(imgs).cuda(), torch.from_numpy(masks).cuda()


def _expected(imgs, masks, src, p, dx=None, dy=None):
    i, m = ref.augment_with_params(imgs[src].transpose(1, 2, 0), masks[src], p, dx, dy)
    return i.transpose(2, 0, 1), m.astype(np.float32)[None]


@pytest.mark.parametrize("n", [1, 5, 8])
def test_gather_without_elastic_is_bit_exact(n):
    from unet_dc_segmentation_amd.augment import augment_gather, pack_params
    imgs, masks, ci, cm = _cache(3, 40, 40)
    combos = list(itertools.product([False, True], [False, True], range(4), [False, True]))
    r = np.random.default_rng(n)
    for b0 in range(0, len(combos), n):
        ps = [dict(hflip=hf, vflip=vf, k=k, bc=bc, alpha=1.0 + r.uniform(-0.2, 0.2) if bc else 1.0,
                   beta=r.uniform(-0.2, 0.2) if bc else 0.0, elastic=False, field_seed=0)
              for hf, vf, k, bc in combos[b0:b0 + n]]
        src = [int(v) for v in r.integers(0, 3, len(ps))]
        rec, seeds = pack_params(ps, src, [float(imgs[s].max()) for s in src])
        assert len(seeds) == 0
        oi, om = augment_gather(ci, cm, rec)
        oi, om = oi.cpu().numpy(), om.cpu().numpy()
        for j, (p, s) in enumerate(zip(ps, src)):
            ei, em = _expected(imgs, masks, s, p)
            assert np.array_equal(oi[j].view(np.uint32), ei.view(np.uint32)), (p, s)
            assert np.array_equal(om[j], em), (p, s)


def test_gather_non_square_even_k_and_odd_k_rejected():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.augment import augment_gather, pack_params
    imgs, masks, ci, cm = _cache(2, 24, 36)
    ps = [dict(hflip=True, vflip=True, k=2, bc=True, alpha=0.9, beta=0.1, elastic=False, field_seed=0),
          dict(hflip=False, vflip=True, k=0, bc=False, alpha=1.0, beta=0.0, elastic=False, field_seed=0)]
    rec, _ = pack_params(ps, [1, 0], [float(imgs[1].max()), float(imgs[0].max())])
    oi, om = augment_gather(ci, cm, rec)
    for j, s in enumerate([1, 0]):
        ei, em = _expected(imgs, masks, s, ps[j])
        assert np.array_equal(oi[j].cpu().numpy(), ei) and np.array_equal(om[j].cpu().numpy(), em)
    ps[1]["k"] = 3
    rec, _ = pack_params(ps, [1, 0], [1.0, 1.0])
    with pytest.raises(_lib.UnetdcError, match="square"):
        augment_gather(ci, cm, rec)


@pytest.mark.parametrize("alpha,sigma", [(1.0, 50.0), (300.0, 10.0)])
def test_gather_elastic_matches_map_coordinates(alpha, sigma):
    from unet_dc_segmentation_amd.augment import augment_gather, elastic_fields, pack_params
    s = 192
    imgs, masks, ci, cm = _cache(3, s, s, seed=9)
    r = np.random.default_rng(int(alpha))
    ps = []
    for j in range(5):
        bc = j % 2 == 1
        ps.append(dict(hflip=bool(j & 1), vflip=bool(j & 2), k=j % 4, bc=bc, alpha=1.0 + r.uniform(-0.2, 0.2) if bc else 1.0,
                       beta=r.uniform(-0.2, 0.2) if bc else 0.0, elastic=j != 2, field_seed=int(r.integers(0, 2 ** 32))))
    src = [j % 3 for j in range(5)]
    rec, seeds = pack_params(ps, src, [float(imgs[i].max()) for i in src])
    fields = elastic_fields(seeds, s, s, sigma, alpha)
    oi, om = augment_gather(ci, cm, rec, fields)
    oi, om, fh = oi.cpu().numpy(), om.cpu().numpy(), fields.cpu().numpy().astype(np.float64)
    assert np.abs(fh).max() > (1.0 if alpha > 1 else 1e-4)
    yy, xx = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    for j, p in enumerate(ps):
        if not p["elastic"]:
            ei, em = _expected(imgs, masks, src[j], p)
            assert np.array_equal(oi[j], ei) and np.array_equal(om[j], em)
            continue
        dx, dy = fh[rec[j]["field"], 0], fh[rec[j]["field"], 1]
        ei, em = _expected(imgs, masks, src[j], p, dx, dy)
        assert np.abs(oi[j] - ei).max() <= 5e-5, (j, np.abs(oi[j] - ei).max())
        frac = lambda c: np.abs((c - np.floor(c)) - 0.5)                     # noqa: E731
        near_tie = (frac(yy + dy) < 1e-3) | (frac(xx + dx) < 1e-3)
        diff = om[j][0] != em[0]
        assert not (diff & ~near_tie).any(), (j, int(diff.sum()), int(near_tie.sum()))


# ---- launch chunks, geometry edges and out-of-view writes: every output and the workspace sit between canaries, the workspace
# at exactly the size unetdc_elastic_fields_workspace declares ------------------------------------------------------------------
def _fields_canaried(seeds, h, w, sigma, alpha):
    from unet_dc_segmentation_amd.augment import elastic_fields, fields_workspace_bytes
    n = len(seeds)
    out, ws = Canaried(n * 2 * h * w * 4), Canaried(fields_workspace_bytes(n, h, w, sigma))
    f = elastic_fields(np.array(seeds, dtype=np.uint32), h, w, sigma, alpha, out=out.view(torch.float32, n, 2, h, w), workspace=ws.u8)
    torch.cuda.synchronize()
    out.check("fields")
    ws.check("fields workspace")
    return f


def _gather_canaried(ci, cm, rec, fields=None):
    from unet_dc_segmentation_amd.augment import augment_gather
    n, (_, c, h, w) = len(rec), ci.shape
    oi, om = Canaried(n * c * h * w * 4), Canaried(n * h * w * 4)
    augment_gather(ci, cm, rec, fields, out_img=oi.view(torch.float32, n, c, h, w), out_mask=om.view(torch.float32, n, 1, h, w))
    torch.cuda.synchronize()
    oi.check("augmented images")
    om.check("augmented masks")
    return oi.numpy(np.float32, n, c, h, w), om.numpy(np.float32, n, 1, h, w)


def _assert_elastic_sample(oi, om, ei, em, dx, dy, what):
    """The module's elastic tolerances: image <= 5e-5, mask equal outside the near-tie set, which may cover at most 2 %."""
    assert np.abs(oi - ei).max() <= 5e-5, (what, np.abs(oi - ei).max())
    tie = fx.near_tie(dx, dy)
    assert tie.mean() <= fx.NEAR_TIE_CAP, (what, tie.mean())
    diff = om[0] != em[0]
    assert not (diff & ~tie).any(), (what, int(diff.sum()), int(tie.sum()))


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("n", [32, 33, 70])
def test_gather_across_the_launch_chunk_is_bit_exact(n, c):
    """launch_augment_gather issues one launch per AUG_MAX_BATCH = 32 records and tells each its first sample (n0): every
    sample, sample 32 and the last one included, must land in its own output slot with its own record."""
    from unet_dc_segmentation_amd.augment import pack_params
    imgs, masks, ci, cm = _cache(5, 40, 40, seed=n, c=c)
    ps, src = fx.chunk_params(n, 5, seed=100 + n)
    rec, seeds = pack_params(ps, src, [float(imgs[s].max()) for s in src])
    assert len(seeds) == 0 and len(rec) == n
    oi, om = _gather_canaried(ci, cm, rec)
    for j, (p, s) in enumerate(zip(ps, src)):
        ei, em = _expected(imgs, masks, s, p)
        assert np.array_equal(oi[j].view(np.uint32), ei.view(np.uint32)), (j, p, s)
        assert np.array_equal(om[j], em), (j, p, s)


@pytest.mark.parametrize("n", [64, 65, 130])
def test_fields_across_the_seed_chunk(n):
    """launch_elastic_fields issues its two passes per AUG_MAX_SEEDS = 64 seeds and tells both the first slot (slot0)."""
    h, w, sigma = 48, 72, 3.0
    seeds = fx.field_seeds(n)
    f = _fields_canaried(seeds, h, w, sigma, 1.0).cpu().numpy()
    for i, s in enumerate(seeds):
        for c, want in enumerate(ref.fields(s, h, w, sigma, 1.0)):
            err = np.abs(f[i, c] - want).max()
            assert err <= 1e-5 * np.abs(want).max(), (i, s, c, err, np.abs(want).max())
    if n == 130:
        assert not np.array_equal(f[0], f[64]) and not np.array_equal(f[0], f[129]) and not np.array_equal(f[64], f[129])


@pytest.mark.parametrize("case", sorted(fx.ELASTIC_CASES))
def test_gather_elastic_across_chunks_and_long_displacements(case):
    """chunks: 70 samples, 66 elastic -- the field slot of a sample behind the first gather launch is the number of elastic
    samples before it, and slots 64, 65 come from the second field launch.  long: |d| > 2 H for part of the field, so
    aug_reflect wraps more than one period.  Reference: augment_ref (scipy.ndimage.map_coordinates, mode="reflect")."""
    from unet_dc_segmentation_amd.augment import pack_params
    n, elastic, s, sigma, alpha = fx.ELASTIC_CASES[case]
    imgs, masks, ci, cm = _cache(5, s, s, seed=21)
    ps, src = fx.chunk_params(n, 5, seed=7, elastic=elastic)
    rec, seeds = pack_params(ps, src, [float(imgs[i].max()) for i in src])
    assert len(seeds) == len(elastic)
    fields = _fields_canaried(seeds, s, s, sigma, alpha)
    oi, om = _gather_canaried(ci, cm, rec, fields)
    fh = fields.cpu().numpy().astype(np.float64)
    if case == "long":
        assert (np.abs(fh) > 2 * s).mean() > 0.05
    slot = 0
    for j, p in enumerate(ps):
        if not p["elastic"]:
            ei, em = _expected(imgs, masks, src[j], p)
            assert np.array_equal(oi[j], ei) and np.array_equal(om[j], em), j
            continue
        assert rec[j]["field"] == slot and seeds[slot] == p["field_seed"]
        dx, dy = fh[slot, 0], fh[slot, 1]
        ei, em = _expected(imgs, masks, src[j], p, dx, dy)
        _assert_elastic_sample(oi[j], om[j], ei, em, dx, dy, (case, j, slot))
        slot += 1
    assert slot == len(seeds) and (case != "chunks" or slot > fx.FIELDS_MAX_SEEDS)


def test_gather_elastic_on_a_non_square_image():
    """The elastic branch with H != W (24 x 40): the taps reflect at the border of their OWN axis.  An odd k is refused on a
    non-square image, so k is 0 or 2; both flips and brightness / contrast are on in two records each.  sigma = 3, alpha = 40
    (the values of the crop tests for small windows) move rows past both borders of the 24-row axis."""
    from unet_dc_segmentation_amd.augment import pack_params
    h, w, sigma, alpha = 24, 40, 3.0, 40.0
    imgs, masks, ci, cm = _cache(2, h, w, seed=31)
    ps = [dict(hflip=bool(j & 1), vflip=bool(j & 2), k=(0, 2, 2, 0)[j], bc=j in (1, 2), alpha=(1.0, 1.15, 0.85, 1.0)[j],
               beta=(0.0, -0.1, 0.12, 0.0)[j], elastic=True, field_seed=(1, 2, 2, 1)[j]) for j in range(4)]
    src = [0, 1, 0, 1]
    rec, seeds = pack_params(ps, src, [float(imgs[s].max()) for s in src])
    assert list(seeds) == [1, 2, 2, 1] and list(rec["field"]) == [0, 1, 2, 3]
    fields = _fields_canaried(seeds, h, w, sigma, alpha)
    oi, om = _gather_canaried(ci, cm, rec, fields)
    fh = fields.cpu().numpy().astype(np.float64)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for j, p in enumerate(ps):
        dx, dy = fh[j]
        for c, want in enumerate(ref.fields(p["field_seed"], h, w, sigma, alpha)):
            assert np.abs(fh[j, c] - want).max() <= 1e-5 * np.abs(want).max(), (j, c)
        if p["field_seed"] == 1:
            assert (yy + dy).min() < -1 and (yy + dy).max() > h and ((xx + dx).min() < -1 or (xx + dx).max() > w)
        ei, em = _expected(imgs, masks, src[j], p, dx, dy)
        _assert_elastic_sample(oi[j], om[j], ei, em, dx, dy, (j, p))


def test_long_displacements_match_map_coordinates_directly():
    """The long-displacement fixture once more without flips, rotation or brightness, against a plain
    scipy.ndimage.map_coordinates call (no code of augment_ref between the kernel and SciPy)."""
    from unet_dc_segmentation_amd.augment import pack_params
    _, _, s, sigma, alpha = fx.ELASTIC_CASES["long"]
    imgs, masks, ci, cm = _cache(2, s, s, seed=22)
    p = dict(hflip=False, vflip=False, k=0, bc=False, alpha=1.0, beta=0.0, elastic=True, field_seed=0xC0FFEE)
    rec, seeds = pack_params([p], [1], [1.0])
    fields = _fields_canaried(seeds, s, s, sigma, alpha)
    oi, om = _gather_canaried(ci, cm, rec, fields)
    dx, dy = fields.cpu().numpy().astype(np.float64)[0]
    assert (np.abs(dy) > 2 * s).any() and (np.abs(dx) > 2 * s).any()
    yy, xx = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    ei = np.stack([ndimage.map_coordinates(imgs[1, c], [yy + dy, xx + dx], order=1, mode="reflect") for c in range(3)])
    em = ndimage.map_coordinates(masks[1], [yy + dy, xx + dx], order=0, mode="reflect").astype(np.float32)[None]
    _assert_elastic_sample(oi[0], om[0], ei.astype(np.float32), em, dx, dy, "direct")


@pytest.mark.parametrize("h,w,sigma", [(37, 600, 3.0), (30, 1023, 2.0), (1, 300, 2.0), (300, 1, 2.0), (1024, 40, 2.0),
                                       (40, 1024, 2.0), (1, 1, 1.0), (50, 70, 20.0)])
def test_fields_geometry_edges(h, w, sigma):
    """H not a multiple of AUG_ROWS = 4 or of 32; 512 < W < 1024 (a second, partial 512-column turn of the row pass); one-row
    and one-column fields; a side at AUG_MAX_SIDE; the radius beyond both sides."""
    seeds = [h * 131 + w, 2 ** 32 - 1 - w]
    f = _fields_canaried(seeds, h, w, sigma, 2.5).cpu().numpy()
    for i, s in enumerate(seeds):
        for c, want in enumerate(ref.fields(s, h, w, sigma, 2.5)):
            err = np.abs(f[i, c] - want).max()
            assert err <= 1e-5 * np.abs(want).max(), (s, c, err, np.abs(want).max())


@pytest.mark.parametrize("h,w", [(1025, 8), (8, 1025)])
def test_fields_side_above_the_maximum_is_rejected(h, w):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.augment import elastic_fields
    out, ws = Canaried(2 * h * w * 4), Canaried(4 * 2 * h * w + 4096)
    with pytest.raises(_lib.UnetdcError, match="sides up to 1024"):
        elastic_fields(np.array([3], dtype=np.uint32), h, w, 2.0, 1.0, out=out.view(torch.float32, 1, 2, h, w), workspace=ws.u8)
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched()


def test_fields_workspace_too_small_is_an_error_before_any_launch():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.augment import fields_workspace_bytes
    h, w, sigma = 20, 30, 3.0
    nbytes = fields_workspace_bytes(2, h, w, sigma)
    out, ws = Canaried(2 * 2 * h * w * 4), Canaried(nbytes)
    seeds = np.array([1, 2], dtype=np.uint32)
    rc = _lib.load().unetdc_elastic_fields(seeds.ctypes.data, 2, h, w, sigma, 1.0, out.ptr, ws.ptr, nbytes - 1,
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -3                                                     # UNETDC_EWORKSPACE
    assert out.untouched() and ws.untouched()
    out.check()
    ws.check()


@pytest.mark.parametrize("h,w", [(30, 50), (5, 530)])
def test_fields_radius_zero_is_alpha_times_noise_bitwise(h, w):
    """sigma = 0.1: int(4 sigma + 0.5) = 0, one tap of weight exactly 1 -- the field is alpha * noise, bit for bit."""
    alpha, seeds = 3.0, [77, 2 ** 31 + 5]
    f = _fields_canaried(seeds, h, w, 0.1, alpha).cpu().numpy()
    for i, s in enumerate(seeds):
        for c in (0, 1):
            want = np.float32(alpha) * ref.noise(s, c, h, w)
            assert want.dtype == np.float32 and np.array_equal(f[i, c].view(np.uint32), want.view(np.uint32)), (s, c)
