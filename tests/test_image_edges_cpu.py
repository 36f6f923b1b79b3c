"""CPU: the constructed inputs of the image-side edge tests (tests/image_edge_fixtures.py) do what their GPU tests rely on, and
the canary helper (tests/image_canaries.py) catches a flipped byte on either side of a view."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import augment_ref as ref
from tests import image_edge_fixtures as fx
from tests.image_canaries import CANARY, Canaried, canaried_like


# ---- the canary helper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes,align,skew", [(1, 16, 0), (100, 16, 0), (4096, 256, 0), (37, 16, 4), (64, 64, 63), (0, 16, 0)])
def test_canaried_view_has_the_size_and_alignment_asked_for(nbytes, align, skew):
    c = Canaried(nbytes, align=align, skew=skew, device="cpu")
    assert c.u8.numel() == nbytes and c.ptr % align == skew and (nbytes == 0 or c.u8.data_ptr() == c.ptr)
    assert c.start >= 512 and c.buf.numel() - c.start - nbytes >= 512
    assert c.untouched()
    c.check()
    c.u8.fill_(7)                                           # writing all of the view, and only the view, passes
    c.check()
    assert nbytes == 0 or not c.untouched()


@pytest.mark.parametrize("where", ["first_below", "last_below", "first_above", "last_above"])
def test_one_flipped_byte_outside_the_view_is_caught(where):
    c = Canaried(40, align=16, device="cpu")
    i = {"first_below": 0, "last_below": c.start - 1, "first_above": c.start + 40, "last_above": c.buf.numel() - 1}[where]
    c.buf[i] = CANARY ^ 1
    with pytest.raises(AssertionError, match="below" if "below" in where else "above"):
        c.check()


def test_canaried_typed_views_and_copies():
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    c = canaried_like(a, align=16, device="cpu")
    assert torch.equal(c.view(torch.float32, 2, 3, 4), torch.from_numpy(a)) and np.array_equal(c.numpy(np.float32, 2, 3, 4), a)
    c.view(torch.float32, 24)[23] = -1.0
    c.check()
    assert c.numpy(np.float32, 24)[23] == -1.0
    m = canaried_like(np.arange(7, dtype=np.uint8), align=16, skew=4, device="cpu")
    assert m.ptr % 16 == 4 and list(m.numpy(np.uint8, 7)) == list(range(7))


# ---- rolling ball: the tie image -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("k", [3, 5, 50])
def test_tie_image_tells_half_even_from_half_up(k, channels):
    from utils.data_loader import rolling_ball_correction_rgb
    img = fx.tie_image(channels)
    out = rolling_ball_correction_rgb(img, k)
    for c in range(channels):
        pos = fx.tie_positions(img, c)
        assert sorted(pos) == list(range(1, 11))
        got = [int(out[pos[v] + (c,)]) for v in range(1, 11)]
        assert got == fx.TIE_EXPECTED == [26, 51, 76, 102, 128, 153, 178, 204, 230, 255]
        assert 76 in out[..., c] and 178 in out[..., c] and 77 not in out[..., c] and 179 not in out[..., c]
        # the same arithmetic rounded half up differs exactly at the two ties
        v = np.arange(1, 11).astype(np.float32) * np.float32(25.5)
        assert [int(x) for x in np.floor(v + np.float32(0.5))] == fx.TIE_HALF_UP != fx.TIE_EXPECTED
        assert int((out[..., c] > 0).sum()) == 10               # nothing but the ten pixels survives the opening


# ---- augmentation: chunk crossings and the near-tie cap ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 33, 70])
def test_gather_chunk_batches_cross_the_launch_and_do_not_repeat_with_it(n):
    from unet_dc_segmentation_amd.augment import pack_params
    ps, src = fx.chunk_params(n, 5, seed=100 + n)
    rec, seeds = pack_params(ps, src, [1.0] * n)
    assert len(rec) == n and len(seeds) == 0 and (n > fx.GATHER_MAX_BATCH) == (n != 32)
    key = [(p["hflip"], p["vflip"], p["k"], p["bc"], s) for p, s in zip(ps, src)]
    if n > fx.GATHER_MAX_BATCH:                              # a launch that reused chunk 0's records would be seen
        assert key[fx.GATHER_MAX_BATCH:] != key[:n - fx.GATHER_MAX_BATCH]
        assert key[32] != key[0] and key[-1] != key[(n - 1) % 32]
    assert {p["k"] for p in ps} == {0, 1, 2, 3} and {p["hflip"] for p in ps} == {p["vflip"] for p in ps} == {False, True}
    assert set(src) == set(range(5)) and {p["bc"] for p in ps} == {False, True}


@pytest.mark.parametrize("n", [64, 65, 130])
def test_field_seed_batches(n):
    seeds = fx.field_seeds(n)
    assert len(set(seeds)) == n and all(0 <= s < 2 ** 32 for s in seeds) and (n > fx.FIELDS_MAX_SEEDS) == (n != 64)
    if n == 130:
        a, b, c = (ref.noise(seeds[i], 0, 4, 8) for i in (0, 64, 129))
        assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


@pytest.mark.parametrize("case", sorted(fx.ELASTIC_CASES))
def test_elastic_fixtures_cross_the_chunks_and_stay_under_the_near_tie_cap(case):
    from unet_dc_segmentation_amd.augment import pack_params
    n, elastic, s, sigma, alpha = fx.ELASTIC_CASES[case]
    ps, src = fx.chunk_params(n, 5, seed=7, elastic=elastic)
    rec, seeds = pack_params(ps, src, [1.0] * n)
    assert len(seeds) == len(elastic) == int((rec["field"] >= 0).sum())
    if case == "chunks":
        assert n >= 40 and len(seeds) >= 33 and n > fx.GATHER_MAX_BATCH and len(seeds) > fx.FIELDS_MAX_SEEDS
        later = rec["field"][fx.GATHER_MAX_BATCH:]
        assert later.max() >= fx.FIELDS_MAX_SEEDS and (later == -1).any()
        assert rec["field"][fx.GATHER_MAX_BATCH] != 0 and rec["field"][fx.GATHER_MAX_BATCH] != fx.GATHER_MAX_BATCH
    far = 0.0
    for seed in seeds:
        dx, dy = ref.fields(int(seed), s, s, sigma, alpha)
        assert fx.near_tie(dx, dy).mean() <= fx.NEAR_TIE_CAP, (case, int(seed), fx.near_tie(dx, dy).mean())
        far = max(far, float((np.abs(dy) > 2 * s).mean()), float((np.abs(dx) > 2 * s).mean()))
    assert (far > 0.05) == (case == "long")


def test_long_direct_fixture_stays_under_the_near_tie_cap():
    _, _, s, sigma, alpha = fx.ELASTIC_CASES["long"]
    dx, dy = ref.fields(0xC0FFEE, s, s, sigma, alpha)
    assert fx.near_tie(dx, dy).mean() <= fx.NEAR_TIE_CAP
    assert (np.abs(dy) > 2 * s).any() and (np.abs(dx) > 2 * s).any()


def test_loader_fixture_fields_stay_under_the_near_tie_cap():
    """The small-cache loader tests (tests/test_gpu_device_data.py: 64 x 64, sigma 4, alpha 8) for every field seed they draw."""
    from unet_dc_segmentation_amd.augment import draw_params
    worst, count = 0.0, 0
    for seed, ids in ((11, range(40)), (11, [3 * i + 1000 for i in range(40)]), (5, range(40))):
        for epoch in (0, 1):
            for i in ids:
                p = draw_params(seed, epoch, i)
                if p["elastic"]:
                    dx, dy = ref.fields(p["field_seed"], 64, 64, 4.0, 8.0)
                    worst, count = max(worst, float(fx.near_tie(dx, dy).mean())), count + 1
                    assert 0.3 < np.abs(dx).max() < 3.0
    assert count >= 30 and worst <= fx.NEAR_TIE_CAP


def test_radius_zero_sigma():
    """sigma = 0.1 gives scipy's radius int(4 sigma + 0.5) = 0: the filter is the identity."""
    assert int(4 * 0.1 + 0.5) == 0
    dx, _ = ref.fields(77, 6, 9, 0.1, 3.0)
    assert np.array_equal(dx, ref.noise(77, 0, 6, 9).astype(np.float64) * 3.0)


# ---- connected components: the area-boundary mask --------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", [2, 5])
def test_area_boundary_mask_components(min_area):
    m = fx.area_boundary_mask(min_area)
    assert m.shape[1] % 4 != 0
    lab, n = ndimage.label(m)
    areas = np.bincount(lab.ravel())[1:]
    assert n == 9 and sorted(areas) == [min_area - 1] * 3 + [min_area] * 3 + [min_area + 1] * 3
    flat = m.ravel()
    ends = np.flatnonzero(flat[:-1] & flat[1:] & (np.arange(1, flat.size) % m.shape[1] == 0))
    assert len(ends) == 3                                   # set pixels adjacent in memory across a row end, yet separate
    for e in ends:
        assert lab.ravel()[e] != lab.ravel()[e + 1]
    first = [int(np.flatnonzero(lab.ravel() == i)[0]) for i in range(1, n + 1)]
    assert first == sorted(first)
