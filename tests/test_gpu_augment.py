"""GPU: the augmentation kernels (csrc/augment.hip) against the numpy restatement in tests/augment_ref.py -- displacement
fields against scipy.ndimage.gaussian_filter of the restated noise, the gather bit-exact without elastic and within float32
interpolation error with it."""
import itertools

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import augment_ref as ref

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


def _cache(m, h, w, seed=0):
    r = np.random.default_rng(seed)
    imgs = (r.integers(0, 256, (m, 3, h, w)) / 255.0).astype(np.float32)
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
