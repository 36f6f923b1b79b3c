"""GPU: the shared wave and workgroup helpers of csrc/wave_ops.h through the stages that use them, each against its existing host
path, bit for bit.

  runs    wave_runs / run_mask / run_sum, run_min, run_max and row_unit serve five per-row stages.  The map of
          tests/droplet_edge_fixtures.py:run_edge_labels puts every edge of a run on one 6 x 130 image (a run over all 64 lanes,
          64 heads in a wave, changes exactly at the chunk seams, a label in the last of 2 live lanes, a run split by a label
          out of range); its first column and its first 65 columns are the widths 1 and 65.
  scans   spatial_window_scan_kernel is scan_plane over the window's row counts, 256 rows a trip: windows of n x 3 random bits
          with n around one trip, four trips and their successors.  Every simulated point is drawn through the row prefix, so
          1024 points in 7 simulations land on every row several times.  (The emit kernels' block_excl_scan cases are in
          tests/test_gpu_droplets.py and tests/test_gpu_diffmap.py, next to the tests of those stages.)"""
import numpy as np
import pytest

from tests import droplet_edge_fixtures as fx
from tests.test_confidence_cpu import BAND, THRESH, planes
from tests.test_gpu_boundary import assert_same as assert_boundary_same
from tests.test_gpu_boundary import device_boundary
from tests.test_gpu_confidence import assert_equals_host as assert_confidence_equals_host
from tests.test_gpu_confidence import device_confidence
from tests.test_gpu_hull import assert_equals_ref as assert_hull_equals_ref
from tests.test_gpu_hull import device_hull
from tests.test_gpu_match import assert_equals_host_path as assert_overlap_equals_host_path
from tests.test_gpu_shape import assert_props_equal
from tests.test_gpu_spatial import assert_counts_equal_host
from tests.test_shape_cpu import gray_plane
from utils import droplet_boundary as db
from utils import droplet_hull as dh

pytestmark = pytest.mark.gpu

K = fx.RUN_EDGE_MAX_OUT


def props(lab):
    h, w = lab.shape
    assert_props_equal(lab, gray_plane(h, w, seed=w), max_out=K)


def confidence(lab):
    h, w = lab.shape
    p, lo, hi = planes(h, w, seed=w)
    got = device_confidence(lab, p, THRESH, BAND, lo, hi, max_out=K, maps=True)
    assert_confidence_equals_host(got, lab, p, THRESH, BAND, lo, hi, max_out=K)


def overlap(lab):
    assert_overlap_equals_host_path(lab, K, fx.moved_one_pixel(lab), K)


def hull(lab):
    rows, _, _ = device_hull(lab, K)
    assert_hull_equals_ref(rows, dh.label_hull_numpy(lab, K))


def boundary(lab):
    moved = fx.moved_one_pixel(lab)
    assert_boundary_same(device_boundary(lab, K, moved, K, 4), db.boundary_record_numpy(lab, K, moved, K, 4))


@pytest.mark.parametrize("width", [130, 1, 65])
@pytest.mark.parametrize("stage", [props, confidence, overlap, hull, boundary], ids=lambda f: f.__name__)
def test_run_edges_equal_the_host_path(stage, width):
    stage(np.array(fx.run_edge_labels()[:, :width], order="C"))             # a writable, contiguous copy


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_window_prefix_around_the_scan_trips(n):
    rng = np.random.default_rng(n)
    window = rng.integers(0, 2, (n, 3)).astype(np.uint8)
    N = 1024
    py, px = rng.integers(0, n, N), rng.integers(0, 3, N)
    want = assert_counts_equal_host(py, px, n, 3, 8, 7, 11, window)
    if window.any():
        assert all(int(want[0][s][0]) == N for s in range(8))       # every simulation drew its N points
