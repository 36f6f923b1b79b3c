"""GPU: the grid-stride loops of the droplet stages on their second trip.  A launcher caps its grid; past the cap a thread
(or a wave) comes round again with `index += stride`.  Per capped kernel: the cap, and the test whose shape exceeds it.

  label_props_kernel (shape.hip)        8192 blocks x 4 waves = 32 768 units of 64 pixels of a row.  8200 x 257 (5 units per row,
                                        the last of one pixel: 41 000 units) and 600 x 3521 (56 per row, the last of one pixel:
                                        33 600 units): test_label_props_past_the_grid_cap.
  match_overlap_kernel (match.hip)      the same cap and shapes: test_label_overlap_past_the_grid_cap.
  label_props_init_kernel (shape.hip)   1024 blocks x 256 threads = 262 144 words, max_out > 18 724: max_out = 20 000 in
                                        test_label_props_initialises_twenty_thousand_numbers (production passes 65 536).
  match_init_kernel, match_compact_kernel (match.hip)   2048 blocks x 256 = 524 288 hash slots.  Already exceeded before this file:
                                        tests/test_gpu_match.py::test_full_size_with_room_for_every_pixel asks for 1 443 520
                                        pairs, that is 4 194 304 slots.  Nothing is added for them; the capacity tests below
                                        exceed the cap too (8 388 608 slots).
  match_sort_global_kernel (match.hip)  4096 blocks x 256 = 1 048 576 compare-exchanges, a list padded past 2^21 entries.  The
                                        test named above pads to exactly 2^21: one trip.  600 x 3521 and 8200 x 257 with
                                        max_pairs = h * w pad to 2^22: test_label_overlap_with_room_for_every_pixel.
  the per-pixel loops of split.hip, clean.hip, ccl.hip, density.hip   4096 blocks x 256 = 1 048 576 pixels: exceeded by every
                                        1040 x 1388 test of tests/test_gpu_split.py, test_gpu_clean.py, test_gpu_shape.py and
                                        test_gpu_density.py.

The label maps (tests/droplet_edge_fixtures.py:cap_labels) are the components of a blob mask: a few hundred droplets that
cross the 64-pixel seams, some of them the row where the second trip starts, and one in the last rows and columns.  Host
references at these shapes, timed on the CPU: label_props_numpy 0.25 s, overlap_table_numpy 0.03 s, the plain loops of
tests/match_ref.py 0.5 s -- the shapes the cap asks for are kept."""
import numpy as np
import pytest

from tests import droplet_edge_fixtures as fx
from tests.match_ref import overlap_table_ref
from tests.test_gpu_match import device_overlap, host_table
from tests.test_gpu_shape import NQ, assert_props_equal
from tests.test_match_cpu import kmax
from tests.test_shape_cpu import gray_plane
from utils import droplet_shape as sh

pytestmark = pytest.mark.gpu

IDS = [f"{h}x{w}" for h, w in fx.CAP_SHAPES]
_plain = {}


def plain_table(shape):
    """The contingency table by the plain loops of tests/match_ref.py, once per shape."""
    if shape not in _plain:
        A, B = fx.cap_labels(shape)
        _plain[shape] = overlap_table_ref(A.tolist(), B.tolist(), kmax(A), kmax(B))
    return _plain[shape]


def assert_reaches_the_second_trip(lab):
    h, w = lab.shape
    assert h * ((w + 63) // 64) > fx.WAVE_UNITS_PER_TRIP and w % 64 == 1
    late = fx.labels_past_unit(lab)
    assert len(late) >= 1                                                  # a labelled run in a unit >= 32 768
    assert len(np.intersect1d(late, fx.labels_before_unit(lab))) >= 1      # a droplet on both sides of the trip boundary
    assert ((lab[:, 63] == lab[:, 64]) & (lab[:, 63] > 0)).any()           # ... and across a 64-pixel seam
    assert lab[h - 1, w - 1] > 0                                           # the last unit holds one pixel, and it is labelled


@pytest.mark.parametrize("with_gray", [False, True], ids=["no_gray", "gray"])
@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_label_props_past_the_grid_cap(shape, with_gray):
    lab = fx.cap_labels(shape)[0]
    assert_reaches_the_second_trip(lab)
    assert_props_equal(lab, gray_plane(*shape, seed=5) if with_gray else None)


def test_label_props_initialises_twenty_thousand_numbers():
    """max_out = 20 000: 280 000 words, the init kernel's second trip.  Every row past the last label holds its initial value."""
    lab = fx.few_dozen_labels()
    k = kmax(lab)
    assert 24 <= k <= 100 and NQ * 20000 > 1024 * 256
    for gray in (None, gray_plane(*lab.shape)):
        got = assert_props_equal(lab, gray, max_out=20000)
        assert np.array_equal(got[:, k:], fx.initial_rows(NQ, 20000 - k, sh.QUANTITIES, sh.MIN_INIT, sh.MAX_INIT))


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_label_overlap_past_the_grid_cap(shape):
    """A capacity of a few thousand pairs: the overlap kernel alone is past its cap."""
    A, B = fx.cap_labels(shape)
    assert_reaches_the_second_trip(A)
    assert_reaches_the_second_trip(B)
    ka, kb = kmax(A), kmax(B)
    ref = host_table(A, ka, B, kb)
    assert ref == plain_table(shape) and 200 <= len(ref) <= 999
    assert device_overlap(A, ka, B, kb, max_pairs=4 * (ka + kb) + 64) == (len(ref), ref)


@pytest.mark.parametrize("shape", fx.CAP_SHAPES, ids=IDS)
def test_label_overlap_with_room_for_every_pixel(shape):
    """max_pairs = h * w > 2^21: 2^23 hash slots (init and compact on their second trip) and a list padded to 2^22 entries, so
    every global compare-exchange pass of the sort takes a second trip over its 2^21 pairs."""
    A, B = fx.cap_labels(shape)
    h, w = shape
    assert 1 << 21 < h * w <= 1 << 22
    ka, kb = kmax(A), kmax(B)
    assert device_overlap(A, ka, B, kb) == (len(plain_table(shape)), plain_table(shape))
