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
