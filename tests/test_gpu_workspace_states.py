"""GPU: every droplet stage gives the same bytes whatever its workspace held before the call.

droplets.py and density.py allocate one workspace per batch and run clean, then ccl / split, then props, then density through
it, image after image at different sizes: every plane a stage reads was last written by another stage at another geometry.
Here each entry point gets a Canaried view (tests/image_canaries.py) of exactly the bytes its *_workspace query names, in four
states (tests/workspace_states.py): all 0x00, all 0xFF, all 0xA5, and "stale" -- the bytes the stage before it in production
order left at the base of a shared buffer when it ran on a 300 x 401 image:
    clean -> ccl_labels / split_stats / edt -> label_overlap / density_maps -> clean of the next image.
After every call the guards of the workspace and of every output hold, and every output (counts, label planes, the
unetdc_density_stats record) equals the host reference; so it is identical across the four states.

Which kernel initialises which workspace plane (read off the launchers before any of this ran):
  unetdc_mask_clean (clean.hip)   L[n], aux[n]: clean_init_kernel, once before the hysteresis stage and once more before the
                                  hole stage (aux is the seed flag plane first, the area / border word then); the four count
                                  words (out_counts, or aux + n when it is NULL): the first clean_init_kernel of the call, or
                                  clean_copy_kernel on the copy path.
  unetdc_ccl_labels (ccl.hip)     sy[n], sx[n], L[n], area[n]: ccl_init_kernel; blocksum[ceil(n / 1024)]: ccl_count_kernel
                                  writes every entry ccl_scan_kernel reads; rank[n]: ccl_emit_kernel writes it at every kept
                                  root, and ccl_label_kernel reads it at kept roots only.
  unetdc_edt_sq (split.hip)       g[n]: edt_col_kernel writes every pixel of every column before edt_row_kernel reads a row.
  unetdc_split_stats (split.hip)  the ccl planes as above (launch_ccl_init); D2[n]: edt_row_kernel; B[n]: edt_col_kernel (as g),
                                  then split_ascent_kernel rewrites every pixel, then ccl_emit_kernel (as rank, read at kept
                                  roots only).
  unetdc_label_overlap (match.hip) ctl[16], keys[slots], counts[slots], ek[n_sort], ec[n_sort]: match_init_kernel.
  unetdc_density_maps (density.hip) hist[256] and the four min / max words of the record: density_init_kernel; thresh:
                                  density_otsu_kernel; the per-row planes: density_rows_kernel (one block per row, every row);
                                  bounds, maxd2 and the rest of the record: density_rings_kernel; blur, m1, m2, roi, ring,
                                  radial, g0m, g0r, spatial: each written for every pixel by the kernel before its first reader.
  unetdc_label_props (shape.hip)  no workspace; label_props_init_kernel sets all 14 rows of all max_out numbers.
No plane is read before it is written."""
import functools

import numpy as np
import pytest
import torch

from scipy import ndimage

from tests.clean_ref import noise
from tests.image_canaries import Canaried
from tests.test_density_cpu import cell_image
from tests.test_gpu_clean import device_clean
from tests.test_gpu_clean import probs_of as clean_probs
from tests.test_gpu_density import assert_density_equals_host, device_density
from tests.test_gpu_match import device_overlap, host_table
from tests.test_gpu_shape import NQ, assert_props_dicts_equal, device_ccl_labels, device_props, expected_rows, scipy_reference
from tests.test_gpu_split import device_edt, device_split, host_rows
from tests.test_match_cpu import kmax, shift
from tests.test_shape_cpu import cc_labels, gray_plane
from tests.test_split_cpu import noise_mask
from tests.workspace_states import STATES, droplet_table, holds, prepare
from utils import density as hd
from utils import droplet_shape as sh
from utils import droplet_split as ds
from utils.droplet_clean import clean_mask

pytestmark = pytest.mark.gpu

SHAPES = ((37, 53), (96, 130), (276, 408))
STALE_SHAPE = (300, 401)
IDS = [f"{h}x{w}" for h, w in SHAPES]


@functools.lru_cache(maxsize=None)
def mask_of(shape):
    return noise_mask(*shape, seed=shape[0])


@functools.lru_cache(maxsize=None)
def clean_pair(shape):
    weak = mask_of(shape)
    return weak & noise(*shape, shape[0], 0.02), weak


@functools.lru_cache(maxsize=None)
def cell_of(shape):
    return cell_image(*shape, shape[0])


@functools.lru_cache(maxsize=None)
def stale():
    """stage -> the bytes that stage finds at the base of the shared buffer: one buffer of the largest workspace any stage asks
    for at 300 x 401, filled with 0xA5, through which the stages run in production order on a 300 x 401 image."""
    from unet_dc_segmentation_amd import _lib
    lib = _lib.load()
    h, w = STALE_SHAPE
    n = h * w
    size = max(lib.unetdc_mask_clean_workspace(h, w), lib.unetdc_split_workspace(h, w), lib.unetdc_ccl_labels_workspace(h, w),
               lib.unetdc_density_workspace(h, w), lib.unetdc_label_overlap_workspace(h, w, n))
    shared = Canaried(size)

    class Base:                                               # the first `nbytes` of the shared buffer as a call's workspace
        def __init__(self, nbytes):
            self.ptr, self.nbytes = shared.ptr, nbytes

        def check(self, what):
            shared.check(what)
    strong, weak = clean_pair(STALE_SHAPE)
    rgb, cell_mask = cell_of(STALE_SHAPE)
    out = {}
    cleaned, _ = device_clean(strong, weak, 5, ws=Base(lib.unetdc_mask_clean_workspace(h, w)))
    out["after_clean"] = shared.u8.clone()
    _, _, lab = device_split(cleaned, 4, ws=Base(lib.unetdc_split_workspace(h, w)))
    out["after_split"] = shared.u8.clone()
    device_density(rgb, cleaned, 10, 21, planes=False, ws=Base(lib.unetdc_density_workspace(h, w)))
    out["after_density"] = shared.u8.clone()
    device_ccl_labels(cleaned, ws=Base(lib.unetdc_ccl_labels_workspace(h, w)))
    out["after_ccl_labels"] = shared.u8.clone()
    return out


def each_state(nbytes, after):
    """(state, a Canaried view of exactly nbytes in that state, the stale bytes), one per state."""
    assert nbytes > 0
    for state in STATES:
        src = stale()[after] if state == "stale" else None
        yield state, prepare(Canaried(nbytes), state, src), src


def lib():
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_the_stale_states_are_not_a_pattern():
    """The stale bytes differ from stage to stage and hold neither zero pages nor the fill pattern alone."""
    s = stale()
    assert len({int(v[:1 << 20].to(torch.int64).sum()) for v in s.values()}) == len(s)
    for v in s.values():
        head = v[:1 << 20].cpu().numpy()
        assert len(np.unique(head)) > 16


@pytest.mark.parametrize("counts", [True, False], ids=["counts", "no_counts"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mask_clean(shape, counts):
    """Hysteresis and holes together (limit 5: holes filled and holes left open); with out_counts NULL the counts live in the
    workspace.  Stale: what density_maps of the image before left (density -> clean of the next image)."""
    strong, weak = clean_pair(shape)
    m, c = clean_mask(strong, weak, 5)
    assert c[0] > 0 and c[1] + c[3] > 0                       # both stages met something (the smallest mask has one hole, left open)
    for state, ws, _ in each_state(lib().unetdc_mask_clean_workspace(*shape), "after_density"):
        got, gc = device_clean(strong, weak, 5, counts=counts, ws=ws)
        assert np.array_equal(got, m), state
        assert gc == (c.tolist() if counts else None), state


@pytest.mark.parametrize("min_area", [1, 12])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ccl_labels(shape, min_area):
    m = mask_of(shape)
    lab, rows = scipy_reference(m, min_area)
    for state, ws, _ in each_state(lib().unetdc_ccl_labels_workspace(*shape), "after_clean"):
        n, drows, dlab = device_ccl_labels(m, min_area, ws=ws)
        assert n == len(rows) and drows == rows and np.array_equal(dlab, lab), state


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_edt_sq_in_its_documented_workspace(shape):
    """4 * h * w + 64 bytes, as include/unetdc_hip.h promises (less than unetdc_split_workspace, which also covers it)."""
    m = mask_of(shape)
    d = ndimage.distance_transform_edt(m)
    ref = np.rint(d * d).astype(np.int64)
    h, w = shape
    assert 4 * h * w + 64 < lib().unetdc_split_workspace(h, w)
    for state, ws, _ in each_state(4 * h * w + 64, "after_clean"):
        got = device_edt(m, ws=ws)
        assert got.dtype == np.int32 and np.array_equal(got, ref), state


@pytest.mark.parametrize("out_label", [True, False], ids=["label", "no_label"])
@pytest.mark.parametrize("h2", [0, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_split_stats(shape, h2, out_label):
    m = mask_of(shape)
    lab, rows = host_rows(m, h2)
    for state, ws, _ in each_state(lib().unetdc_split_workspace(*shape), "after_clean"):
        n, drows, dlab = device_split(m, h2, labels=out_label, ws=ws)
        assert n == len(rows) and drows == rows, state
        assert np.array_equal(dlab, lab) if out_label else dlab is None, state


@pytest.mark.parametrize("room", ["every_pixel", "just_fits"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_label_overlap(shape, room):
    """Stale: what split_stats left (the label map of the prediction comes from it)."""
    m = mask_of(shape)
    A = ds.split_labels(m, 4, 1)[0]
    B = cc_labels(shift(m, 1, 2))
    ka, kb = kmax(A), kmax(B)
    ref = host_table(A, ka, B, kb)
    assert len(ref) >= 3
    cap = shape[0] * shape[1] if room == "every_pixel" else len(ref)
    for state, ws, _ in each_state(lib().unetdc_label_overlap_workspace(*shape, cap), "after_split"):
        assert device_overlap(A, ka, B, kb, max_pairs=cap, ws=ws) == (len(ref), ref), state
    # one entry too few: the count says so in every state, and nothing is written past the capacity (checked inside)
    for state, ws, _ in each_state(lib().unetdc_label_overlap_workspace(*shape, len(ref) - 1), "after_split"):
        assert device_overlap(A, ka, B, kb, max_pairs=len(ref) - 1, ws=ws)[0] == len(ref), state


@pytest.mark.parametrize("planes", [False, True], ids=["planes_null", "planes_given"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_density_maps(shape, planes):
    """Stale: what clean and then split_stats left.  With the optional planes NULL they live in the workspace."""
    rgb, mask = cell_of(shape)
    ref = hd.density_maps(rgb, mask, 10, 21)
    n = len(droplet_table(mask)[0])
    assert ref["roi_area"] > 0 and ref["ring_counts"].sum() > 0
    first = None
    for after in ("after_split", "after_ccl_labels"):
        for state, ws, _ in each_state(lib().unetdc_density_workspace(*shape), after):
            if after == "after_ccl_labels" and state != "stale":
                continue
            dev = device_density(rgb, mask, 10, 21, planes=planes, ws=ws)
            assert_density_equals_host(dev, ref, 10, n, planes=planes)
            first = first or dev
            assert np.array_equal(dev["stats_bytes"], first["stats_bytes"]), state         # the whole record, byte for byte


def test_a_refused_call_leaves_the_workspace_as_it_was():
    """One byte less than the query: refused before any launch, in every state."""
    shape = SHAPES[0]
    m = mask_of(shape)
    for state, ws, src in each_state(lib().unetdc_split_workspace(*shape) - 1, "after_clean"):
        from unet_dc_segmentation_amd import _lib
        with pytest.raises(_lib.UnetdcError, match="workspace too small"):
            device_split(m, 4, ws=ws)
        torch.cuda.synchronize()
        ws.check("workspace")
        assert holds(ws, state, src), state


@pytest.mark.parametrize("with_gray", [False, True], ids=["no_gray", "gray"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_label_props_output_prefilled(shape, with_gray):
    """No workspace: the [14][max_out] output itself holds each pattern, or the rows of another image, before the call.  Nine
    numbers past the last label have no pixels and must hold the documented initial values."""
    lab = ds.split_labels(mask_of(shape), 4, 1)[0]
    gray = gray_plane(*shape) if with_gray else None
    cap = kmax(lab) + 9
    ref = expected_rows(lab, gray, cap)
    assert np.array_equal(ref[sh.QUANTITIES.index("min_y"), -9:], np.full(9, sh.MIN_INIT))
    assert np.array_equal(ref[sh.QUANTITIES.index("max_x"), -9:], np.full(9, sh.MAX_INIT)) and not ref[0, -9:].any()
    other = ds.split_labels(mask_of(STALE_SHAPE), 4, 1)[0]
    old = torch.from_numpy(np.resize(expected_rows(other, gray_plane(*STALE_SHAPE), kmax(other)), NQ * cap)).cuda()
    for prefill in (0x00, 0xFF, 0xA5, old):
        got = device_props(lab, gray, cap, prefill=prefill)
        for j, q in enumerate(sh.QUANTITIES):
            assert np.array_equal(got[j], ref[j]), (q, prefill if isinstance(prefill, int) else "stale")


# ---- the wrappers: one workspace for a batch of mixed sizes ---------------------------------------------------------------------
BATCH_SIZES = [(64, 64), (300, 401), (97, 33), (96, 130)]
PROBS_SIDE = 128


def batch_probs():
    weak = [noise_mask(PROBS_SIDE, PROBS_SIDE, seed=90 + i, sigma=2.0) for i in range(len(BATCH_SIZES))]
    strong = [wk & noise_mask(PROBS_SIDE, PROBS_SIDE, seed=95 + i, sigma=4.0, frac=0.3) for i, wk in enumerate(weak)]
    return np.stack([clean_probs(s, wk) for s, wk in zip(strong, weak)])


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_mask_and_droplets_batch_equals_single_images_in_either_order(order):
    """Every option on: each image runs clean, split_stats and label_props through the one workspace, after an image of
    another size did; it must return exactly what the image returns alone."""
    from unet_dc_segmentation_amd.droplets import mask_and_droplets, mask_and_droplets_batch
    idx = list(range(len(BATCH_SIZES)))[::1 if order == "forward" else -1]
    sizes = [BATCH_SIZES[i] for i in idx]
    p = batch_probs()[idx]
    probs = torch.from_numpy(p).cuda()
    grays = [torch.from_numpy(gray_plane(h, w, seed=70 + i)).cuda() for i, (h, w) in zip(idx, sizes)]
    opts = dict(split_depth=2.0, shape=True, return_labels=True, thresh_low=0.3, max_hole_area=200)
    out = mask_and_droplets_batch(probs, 0.5, sizes, 1, gray=grays, **opts)
    counts = [o.clean_counts for o in out]
    assert len(out) == len(sizes)
    did = np.zeros(4, np.int64)
    for i, hw in enumerate(sizes):
        one = mask_and_droplets(probs[i], 0.5, hw, 1, gray=grays[i], **opts)
        (mask, a, cy, cx), lab, props = out[i], out[i].labels, out[i].props
        assert torch.equal(one.mask, mask) and torch.equal(one.labels, lab)
        for x, y in zip(list(one)[1:], (a, cy, cx)):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert_props_dicts_equal(one.props, props)
        assert one.clean_counts.shape == (4,) and np.array_equal(one.clean_counts, counts[i])
        assert len(a) > 3 and int(lab.max()) == len(a)
        did += counts[i]
    assert did[0] > 0 and did[1] > 0                           # hysteresis and hole filling both did something


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_density_maps_batch_equals_single_images_in_either_order(order):
    """droplet_sums=None: every image runs ccl_stats and then density_maps through the one workspace."""
    from unet_dc_segmentation_amd.density import density_maps_batch
    sizes = BATCH_SIZES[::1 if order == "forward" else -1]
    cells = [cell_image(h, w, 20 + h) for h, w in sizes]
    rgbs = [torch.from_numpy(r).cuda() for r, _ in cells]
    masks = [torch.from_numpy(m).cuda() for _, m in cells]
    out = density_maps_batch(rgbs, masks, None, 10, 21, planes=True)
    for i, (rgb, m) in enumerate(cells):
        one = density_maps_batch([rgbs[i]], [masks[i]], None, 10, 21, planes=True)[0]
        ref = hd.density_maps(rgb, m, 10, 21)
        assert sorted(one) == sorted(out[i])
        for k, v in out[i].items():
            if torch.is_tensor(v):
                assert torch.equal(v.view(torch.uint8), one[k].view(torch.uint8)), k
            elif isinstance(v, np.ndarray):
                assert np.array_equal(v, one[k]), k
            else:
                assert v == one[k], k
        assert np.array_equal(out[i]["ring_counts"], ref["ring_counts"]) and out[i]["ndroplets"] == len(droplet_table(m)[0])
        for k in ("radial_index", "spatial_index"):
            assert np.array_equal(out[i][k], ref[k]), k
