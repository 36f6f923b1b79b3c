"""CPU: the two records of unet_dc_segmentation_amd/droplets.py -- what a Droplets unpacks to and reaches by name, and the
option combinations DropletOptions refuses.  No device is touched."""
import dataclasses

import numpy as np
import pytest

from unet_dc_segmentation_amd._lib import UnetdcError
from unet_dc_segmentation_amd.droplets import DropletOptions, Droplets


def test_droplets_unpacks_to_four_and_the_rest_is_reached_by_name():
    mask, area = np.ones((3, 4), np.uint8), np.array([12])
    cy, cx = np.array([1.0]), np.array([1.5])
    plain = Droplets(mask, area, cy, cx)
    got = tuple(plain)
    assert len(got) == 4 and all(x is y for x, y in zip(got, (mask, area, cy, cx)))
    m, *rest = plain                                      # the two forms bench.py unpacks
    _, a, y, x = plain
    assert m is mask and len(rest) == 3 and a is area and y is cy and x is cx
    assert plain.labels is None and plain.props is None
    assert plain.clean_counts.dtype == np.int64 and plain.clean_counts.tolist() == [0, 0, 0, 0]
    assert plain.clean_counts is not Droplets(mask, area, cy, cx).clean_counts
    labels, props, counts = np.ones((3, 4), np.int32), {"area": area}, np.array([1, 2, 3, 4])
    full = Droplets(mask, area, cy, cx, labels=labels, props=props, clean_counts=counts)
    assert len(tuple(full)) == 4                          # whatever the options, never more
    assert full.labels is labels and full.props is props and full.clean_counts is counts
    assert full.centroid_row is cy and full.centroid_col is cx
    names = [f.name for f in dataclasses.fields(Droplets)]                 # real fields, behind those of the stages before them
    assert names[names.index("neighbors"):] == ["neighbors", "confidence", "hull"]
    assert all(f.default is None for f in dataclasses.fields(Droplets) if f.name in ("confidence", "hull"))
    assert plain.confidence is None and plain.hull is None
    conf, hull = {"n": area}, {"nv": area}
    both = Droplets(mask, area, cy, cx, confidence=conf, hull=hull)
    assert both.confidence is conf and both.hull is hull and len(tuple(both)) == 4


def today(B, clean, shape, nb, cf, hl):
    """The buffer arithmetic of _droplets as it stood before the layout object, copied: -> the int32 index of (the clean
    counts, the pair counts, the hull's row counts, the int64 totals), the length of counts, the first row of (shape,
    confidence, hull), the rows of sums."""
    NQ, NC, NH = 14, 10, 5
    nc = B * (5 if clean else 1)
    n32 = nc + B * nb + B * hl
    at64 = (n32 + 1) // 2 * 2
    r0 = 2 + NQ * shape
    rh = r0 + NC * cf
    return (B, nc, nc + B * nb, at64), (at64 + 16 * B if cf else n32), (2, r0, rh), rh + NH * hl


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_layout_is_the_arithmetic_it_replaced(B):
    """Every subset of the stages, cleaning on and off: the regions of counts lie in the order count, clean, pairs, hull rows,
    then the int64 totals from an even index; none overlaps another; lengths and row ranges equal the closed forms."""
    import itertools
    from unet_dc_segmentation_amd.droplets import _STAGES, _Layout
    assert [S.field for S in _STAGES] == ["props", "neighbors", "confidence", "hull"]
    for k, clean in itertools.product(range(len(_STAGES) + 1), (False, True)):
        for on in itertools.combinations(_STAGES, k):
            fields = [S.field for S in on]
            shape, nb, cf, hl = (f in fields for f in ("props", "neighbors", "confidence", "hull"))
            lay = _Layout(B, on, clean)
            (at_clean, at_pairs, at_hull, at64), n_counts, (r_shape, r_conf, r_hull), n_rows = today(B, clean, shape, nb, cf, hl)
            assert lay.n_counts == n_counts and lay.n_rows == n_rows and lay.tail == at64 and lay.tail % 2 == 0
            assert lay.n32 <= lay.tail <= lay.n32 + 1
            idx = np.arange(n_counts)
            regions = [lay.int32(idx, "count", i) for i in range(B)] + [lay.int32(idx, "clean", i) for i in range(B)]
            assert regions[0][0] == 0 and [len(r) for r in regions] == [1] * B + [4 * clean] * B
            assert not clean or (regions[B][0] == at_clean and lay.int32(idx, "clean")[-1] == at_clean + 4 * B - 1)
            for f, at in (("neighbors", at_pairs), ("hull", at_hull)):
                if f in fields:
                    regions += [lay.int32(idx, f, i) for i in range(B)]
                    assert [int(r[0]) for r in regions[-B:]] == list(range(at, at + B))
            if cf:                                                   # 8 int64 per image: 16 int32 slots
                i64 = np.arange(n_counts, dtype=np.int32)
                for i in range(B):
                    view = lay.int64(i64, "confidence", i)
                    assert view.dtype == np.int64 and len(view) == 8
                    first = at64 + 16 * i
                    assert view[0] == first + ((first + 1) << 32)   # little endian: the int64 at int32 index `first`
                    regions.append(idx[first:first + 16])
            flat = np.concatenate(regions)
            assert np.array_equal(flat, np.sort(flat)) and len(np.unique(flat)) == len(flat)      # in order, disjoint
            assert len(flat) == n_counts - (at64 - lay.n32 if cf else 0)                           # nothing but the pad is unowned
            rows = np.arange(n_rows)
            want = {"props": (r_shape, 14), "confidence": (r_conf, 10), "hull": (r_hull, 5)}
            got = [lay.rows(rows, f) for f in fields]
            for f, r in zip(fields, got):
                assert list(r) == (list(range(want[f][0], want[f][0] + want[f][1])) if f in want else []), f
            owned = np.concatenate([rows[:2]] + got)
            assert np.array_equal(owned, rows)                        # sum y, sum x, then the stages in order: all rows, once


def test_droplet_options_refuses_the_three_invalid_combinations():
    with pytest.raises(UnetdcError, match="must not exceed"):
        DropletOptions(thresh_low=0.6, thresh=0.5)
    with pytest.raises(UnetdcError, match="return_labels needs"):
        DropletOptions(labels=True)
    with pytest.raises(UnetdcError, match="gray needs"):
        DropletOptions(gray=[np.zeros((3, 4), np.uint8)])
    with pytest.raises(UnetdcError, match="must not exceed"):       # a record built earlier meets its threshold at the call
        dataclasses.replace(DropletOptions(thresh_low=0.6), thresh=0.5)
    ok = DropletOptions(split_depth=1.5, shape=True, labels=True, thresh_low=0.5, max_hole_area=-1, thresh=0.5, gray=[])
    assert (ok.split_depth, ok.shape, ok.labels, ok.thresh_low, ok.max_hole_area) == (1.5, True, True, 0.5, -1)
    assert ok.half_pixels == 3 and ok.cleaning(0.5) == (None, -1) and ok.cleaning(0.7) == (0.5, -1)
    assert DropletOptions(labels=True, split_depth=0.0).half_pixels == 0 and DropletOptions(labels=True, shape=True).labels
    assert DropletOptions().cleaning(0.5) is None and DropletOptions(thresh_low=0.5).cleaning(0.5) is None
    with pytest.raises(dataclasses.FrozenInstanceError):
        ok.shape = False
