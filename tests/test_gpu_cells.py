"""GPU: droplets per cell (csrc/cells.hip) through the C ABI against the brute-force oracle of
tests/cells_ref.py: the nearest-label transform (the tie rule, the radius, the row kernel's thread stride, a row of 16384
pixels in LDS), the per-cell table, both on workspaces and outputs in any state and between canaries; then the stage of
droplets.py with its retry, and the script on the device against its CPU path."""
import functools

import numpy as np
import pytest
import torch

from tests import cells_ref as ref
from tests.image_canaries import Canaried, canaried_like, check_all
from tests.test_cells_cpu import check_refusals, table_d2
from utils import droplet_cells as dc

pytestmark = pytest.mark.gpu

EDT_INF = 2 ** 31 - 1
FILLS = (None, 0xFF, "random")                # what the workspace and the outputs hold on entry: the canary, ones, random bytes


def lib():
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def fill(views, how, seed=0):
    g = torch.Generator().manual_seed(seed)
    for v in views:
        if how == "random":
            v.u8.copy_(torch.randint(0, 256, (v.nbytes,), dtype=torch.uint8, generator=g))
        elif how is not None:
            v.u8.fill_(how)


def device_nearest(label, max_label, radius=0, how=None, ws=None, calls=1):
    """unetdc_label_nearest on a host int32 map -> (label, d2) host planes; every buffer between canaries, the input unchanged."""
    from unet_dc_segmentation_amd._lib import call
    h, w = label.shape
    src = canaried_like(label.astype(np.int32))
    ws = ws or Canaried(lib().unetdc_label_nearest_workspace(h, w))
    out_l, out_d = Canaried(4 * h * w), Canaried(4 * h * w)
    fill((ws, out_l, out_d), how)
    for _ in range(calls):
        call("unetdc_label_nearest", src.ptr, max_label, h, w, radius, ws.ptr, ws.nbytes, out_l.ptr, out_d.ptr, stream())
    torch.cuda.synchronize()
    check_all(src, ws, out_l, out_d)
    assert np.array_equal(src.numpy(np.int32, h, w), label)
    return out_l.numpy(np.int32, h, w), out_d.numpy(np.int32, h, w)


def device_table(drop, md, cell, mc, d2=None, room=None, how=None, ws=None, calls=1):
    """unetdc_cell_table on host maps -> (out_droplet [6, md], out_cell [8, mc], needed)."""
    from unet_dc_segmentation_amd._lib import call
    h, w = drop.shape
    room = h * w if room is None else room
    maps = [canaried_like(np.asarray(m, np.int32)) for m in (drop, cell) + (() if d2 is None else (d2,))]
    ws = ws or Canaried(lib().unetdc_cell_table_workspace(h, w, md, mc, room))
    out_d, out_c, needed = Canaried(4 * 6 * md), Canaried(8 * 8 * mc), Canaried(4)
    fill((ws, out_d, out_c, needed), how)
    for _ in range(calls):
        call("unetdc_cell_table", maps[0].ptr, md, maps[1].ptr, mc, None if d2 is None else maps[2].ptr, h, w, ws.ptr, ws.nbytes,
             needed.ptr, room, out_d.ptr if md else None, out_c.ptr if mc else None, stream())
    torch.cuda.synchronize()
    check_all(*maps, ws, out_d, out_c, needed)
    return out_d.numpy(np.int32, 6, md), out_c.numpy(np.int64, 8, mc), int(needed.numpy(np.int32, 1)[0])


def assert_nearest(label, max_label, radius=0, want=None, **kw):
    got = device_nearest(label, max_label, radius, **kw)
    want = ref.nearest_brute(label, max_label, radius) if want is None else want
    bad = int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum())
    print(f"[cells] nearest {label.shape} radius {radius}: {bad[0]} labels, {bad[1]} distances differ")
    assert bad == (0, 0)
    return got


# ---- nearest label ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.nearest_cases()))
def test_nearest_cases_equal_brute_force(name):
    label, max_label = ref.nearest_cases()[name]
    lab, d2 = assert_nearest(label, max_label)
    if name == "row_tie":                                # the centre pixel ties at 9 and takes label 1
        assert lab.tolist() == [[2, 2, 2, 1, 1, 1, 1]] and d2.tolist() == [[0, 1, 4, 9, 4, 1, 0]]
    if name == "column_tie":
        assert (lab[0:2] == 5).all() and (lab[2:5] == 2).all()
    if name == "no_seed":
        assert (lab == 0).all() and (d2 == EDT_INF).all()
    if name == "all_seeds":
        assert np.array_equal(lab, label) and (d2 == 0).all()


@pytest.mark.parametrize("radius", [1, 3, 0])
def test_radius_cuts_the_label_only(radius):
    label, max_label = ref.nearest_cases()["random_seeds"]
    free = device_nearest(label, max_label, 0)
    lab, d2 = assert_nearest(label, max_label, radius)
    assert np.array_equal(d2, free[1])
    cut = d2 > radius * radius if radius else np.zeros_like(d2, bool)
    assert (lab[cut] == 0).all() and np.array_equal(lab[~cut], free[0][~cut])


@pytest.mark.parametrize("shape", [(1, 1), (1, 64), (64, 255), (64, 256), (64, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smallest_sides_and_the_row_kernels_thread_stride(shape):
    h, w = shape
    n = min(30, h * w)
    assert_nearest(ref.random_seeds(h, w, n, w), n)
    if h == 1:                                           # and without a seed, and with seeds at the ends only
        assert_nearest(np.zeros(shape, np.int32), 3)
        ends = np.zeros(shape, np.int32)
        ends[0, 0], ends[0, -1] = 2, 1
        assert_nearest(ends, 2)


def test_a_row_of_16384_pixels():
    """2 x 16384: both planes of a row fill 128 KiB of LDS.  Seeds at both ends and one in the middle, numbered so that the
    pixels half way tie towards the far side.  Against nearest_label_numpy, which tests/test_cells_cpu.py ties to the brute force."""
    label = np.zeros((2, 16384), np.int32)
    label[0, 0], label[1, 16383], label[0, 8192] = 3, 1, 2
    want = dc.nearest_label_numpy(label, 3)
    lab, d2 = assert_nearest(label, 3, want=want)
    assert set(np.unique(lab)) == {1, 2, 3}
    assert lab[0, 4096] == 2 and d2[0, 4096] == 4096 ** 2            # ties with label 3 at the left end
    assert lab[1, 4096] == 2 and d2[1, 4096] == 4096 ** 2 + 1
    assert_nearest(label, 3, 5000, want=dc.nearest_label_numpy(label, 3, 5000))


@functools.lru_cache(maxsize=None)
def big():
    label = ref.random_seeds(300, 401, 200, 7)
    return label, ref.nearest_brute(label, 200)


@pytest.mark.parametrize("radius", [0, 25])
def test_300x401_with_200_seeds(radius):
    label, (wl, wd) = big()
    want = (wl if radius == 0 else np.where(wd > radius * radius, 0, wl).astype(np.int32)), wd
    lab, _ = assert_nearest(label, 200, radius, want=want)
    assert (lab == 0).any() == (radius > 0)


@pytest.mark.parametrize("name", ["random_seeds", "touching_blocks", "no_seed"])
def test_nearest_does_not_depend_on_what_the_buffers_held(name):
    label, max_label = ref.nearest_cases()[name]
    runs = [device_nearest(label, max_label, 3, how=how) for how in FILLS]
    ws = Canaried(lib().unetdc_label_nearest_workspace(*label.shape))
    runs.append(device_nearest(label, max_label, 3, ws=ws, calls=2))            # two calls in a row on one workspace
    runs.append(device_nearest(label, max_label, 3, ws=ws))                     # and a third on what they left
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
    want = ref.nearest_brute(label, max_label, 3)
    assert np.array_equal(runs[0][0], want[0]) and np.array_equal(runs[0][1], want[1])


def test_refusals_and_a_workspace_one_byte_short_launch_nothing():
    buf = Canaried(4096, align=64)
    check_refusals(lib(), buf.ptr)
    torch.cuda.synchronize()
    assert buf.untouched()
    buf.check("refused calls")


# ---- cell table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_d2", [False, True])
@pytest.mark.parametrize("name", sorted(ref.table_cases()))
def test_table_cases_equal_brute_force(name, with_d2):
    drop, md, cell, mc = ref.table_cases()[name]
    d2 = table_d2(cell, 5) if with_d2 else None
    got, want = device_table(drop, md, cell, mc, d2), ref.cell_table_brute(drop, md, cell, mc, d2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    if name == "mixed":
        assert got[0][0].tolist() == [1, 4, 2, 0, 3, 0, 0] and got[0][2].tolist() == [1, 2, 2, 0, 3, 0, 0]


@functools.lru_cache(maxsize=None)
def droplets_and_cells(h, w, seed):
    """A droplet label map (4-connected components of smooth noise) and territories of random nuclei with their d2."""
    from scipy import ndimage
    from tests.test_split_cpu import noise_mask
    drop = ndimage.label(noise_mask(h, w, seed=seed, sigma=2.0, frac=0.35))[0].astype(np.int32)
    nuclei = ref.random_seeds(h, w, 12, seed)
    cell, d2 = ref.nearest_brute(nuclei, 12, radius=h // 3)
    return drop, int(drop.max()), cell, 12, d2


@pytest.mark.parametrize("shape", [(96, 130), (300, 401)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_table_of_a_droplet_map_over_territories(shape):
    drop, md, cell, mc, d2 = droplets_and_cells(*shape, 5)
    want = dc.cell_table_numpy(drop, md, cell, mc, d2)
    if shape[0] < 100:                                   # the numpy path is tied to the brute force in tests/test_cells_cpu.py, and here
        brute = ref.cell_table_brute(drop, md, cell, mc, d2)
        assert all(np.array_equal(a, b) for a, b in zip(want[:2], brute[:2])) and want[2] == brute[2]
    got = device_table(drop, md, cell, mc, d2)
    assert md > 10 and want[2] > md and (want[0][2] > 1).any() and (want[0][0] == 0).any()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_table_does_not_depend_on_what_the_buffers_held_and_reports_a_room_too_small():
    drop, md, cell, mc, d2 = droplets_and_cells(96, 130, 5)
    want = dc.cell_table_numpy(drop, md, cell, mc, d2)
    room = want[2]                                       # exactly enough
    runs = [device_table(drop, md, cell, mc, d2, room=room, how=how) for how in FILLS]
    ws = Canaried(lib().unetdc_cell_table_workspace(96, 130, md, mc, room))
    runs.append(device_table(drop, md, cell, mc, d2, room=room, ws=ws, calls=2))
    runs.append(device_table(drop, md, cell, mc, d2, room=room, ws=ws))
    for r in runs:
        assert np.array_equal(r[0], want[0]) and np.array_equal(r[1], want[1]) and r[2] == want[2]
    for small in (0, 1, room - 1):                       # "repeat with more room"; nothing is written out of bounds
        assert device_table(drop, md, cell, mc, d2, room=small, how="random")[2] == small + 1


# ---- the stage of droplets.py -----------------------------------------------------------------------------------------------------
def batch_of_three():
    from tests.test_split_cpu import noise_mask
    from unet_dc_segmentation_amd.cells import CellMap, nearest_label
    hws = [(96, 130), (64, 64), (50, 97)]
    probs = np.full((3, 96, 130), 0.1, np.float32)
    for i in range(3):
        probs[i] = np.where(noise_mask(96, 130, seed=20 + i, sigma=2.0, frac=0.35) > 0, 0.9, 0.1)
    maps, host = [], []
    for i, (h, w) in enumerate(hws):
        nuclei = ref.random_seeds(h, w, 5 + 4 * i, 30 + i)
        top = 5 + 4 * i
        if i == 1:                                       # given cells without a d2 plane
            cell = ref.nearest_brute(nuclei, top, 20)[0]
            maps.append(CellMap(torch.from_numpy(cell).cuda(), top, None))
            host.append((cell, top, None))
        else:
            lab, d2 = nearest_label(torch.from_numpy(nuclei).cuda(), top, 25)
            maps.append(CellMap(lab, top, d2))
            host.append((lab.cpu().numpy(), top, d2.cpu().numpy()))
    return torch.from_numpy(probs).cuda(), hws, maps, host


def assert_records_equal(got, want):
    assert set(got) == set(want) and got["nuclei"] == want["nuclei"]
    for q in dc.DROPLET_QUANTITIES:
        assert got[q].dtype == np.int64 and np.array_equal(got[q], want[q]), q
    for q in dc.CELL_QUANTITIES:
        assert got["cells"][q].dtype == np.int64 and np.array_equal(got["cells"][q], want["cells"][q]), q


def test_stage_equals_the_cpu_record_and_its_retry_the_single_large_call(monkeypatch):
    from unet_dc_segmentation_amd import droplets as D
    probs, hws, maps, host = batch_of_three()
    before = D.mask_and_droplets_batch(probs, 0.5, hws, 2, shape=True, return_labels=True)
    out = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, cells=maps)
    triples = []
    for d, b, (cell, top, d2) in zip(out, before, host):
        lab = d.labels.cpu().numpy()
        want = dc.cells_record(lab, len(d.area), cell, top, d2)
        assert_records_equal(d.cells, want)
        assert np.array_equal(d.cells["area"], d.area) and len(d.area) > 3
        triples.append(int(d.cells["n_cells"].sum()))
        # the other fields are those of a call without the option
        assert b.cells is None and torch.equal(d.mask, b.mask) and torch.equal(d.labels, b.labels) and np.array_equal(d.area, b.area)
        assert np.array_equal(d.centroid_row, b.centroid_row) and np.array_equal(d.centroid_col, b.centroid_col)
    # a first room smaller than the triples of every image: each image is run again alone, with twice the room each time
    assert min(triples) > 4
    monkeypatch.setattr(D, "TRIPLE_ROOM", 2)
    again = D.mask_and_droplets_batch(probs, 0.5, hws, 2, return_labels=True, cells=maps)
    for d, a in zip(out, again):
        assert_records_equal(a.cells, d.cells)
        assert torch.equal(a.labels, d.labels)
    monkeypatch.undo()
    one = D.mask_and_droplets(probs[2], 0.5, hws[2], 2, cells=maps[2])
    assert one.labels is None
    assert_records_equal(one.cells, out[2].cells)
    with pytest.raises(D._lib.UnetdcError):
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, cells=maps[:2])
    with pytest.raises(D._lib.UnetdcError):
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, cells=[maps[0]._replace(label=maps[0].label.long())] + maps[1:])


def test_option_off_adds_no_launch_and_no_copy_and_option_on_two_copies(monkeypatch):
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd import droplets as D
    probs, hws, maps, _ = batch_of_three()
    names, copies = [], {"cpu": 0}
    real, real_cpu = _lib.call, torch.Tensor.cpu

    def cpu(self, *a, **k):
        copies["cpu"] += self.is_cuda
        return real_cpu(self, *a, **k)
    monkeypatch.setattr(D._lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    D.mask_and_droplets_batch(probs, 0.5, hws, 2)
    off = list(names)
    assert "unetdc_cell_table" not in off and off.count("unetdc_ccl_stats") == 3 and len(off) == 6     # mask + labelling per image
    assert copies["cpu"] == 3                            # the counts, the areas, the sums: what the batch always waits for
    del names[:]
    D.mask_and_droplets_batch(probs, 0.5, hws, 2, cells=maps)
    assert names.count("unetdc_cell_table") == 3 and names.count("unetdc_ccl_labels") == 3 and len(names) == 9
    assert copies["cpu"] == 3 + 5                        # and the stage's two planes


def test_wrappers_on_the_device():
    from unet_dc_segmentation_amd.cells import cell_table, nearest_label
    drop, md, cell, mc, d2 = droplets_and_cells(96, 130, 5)
    nuclei = ref.random_seeds(96, 130, 12, 5)
    lab, dd = nearest_label(torch.from_numpy(nuclei).cuda(), 12, 32)
    assert np.array_equal(lab.cpu().numpy(), cell) and np.array_equal(dd.cpu().numpy(), d2)
    rec = cell_table(torch.from_numpy(drop).cuda(), md, lab, mc, dd, max_pairs=3)       # grows its room
    assert_records_equal(rec, dc.cells_record(drop, md, cell, mc, d2))


# ---- the script -------------------------------------------------------------------------------------------------------------------
CSVS = ("cells.csv", "cells_per_image.csv", "all_droplets.csv", "summary_per_image.csv")


def test_cli_device_equals_cpu_path_on_fixed_probabilities(tmp_path, monkeypatch):
    """quantify_droplets_batch.py --nuclei_dir / --cell_dir write the same CSVs and territories on the device as on the CPU path,
    given the same probabilities (the network is replaced by fixed maps on both)."""
    import quantify_droplets_batch as q
    from tests.test_cells_cpu import SIZES, cli_probs, write_masks
    from tests.test_split_cpu import files, run_cli
    assert q.DEVICE == "cuda"
    write_masks(tmp_path / "nuc")
    write_masks(tmp_path / "lab", as_labels=True)
    for tag, args in (("n", ["--nuclei_dir", str(tmp_path / "nuc"), "--cell_radius", "20", "--split_touching"]),
                      ("c", ["--cell_dir", str(tmp_path / "lab"), "--cell_labels", "--px_per_micron", "2.0"])):
        dev = run_cli(tmp_path, monkeypatch, "dev" + tag, args, device="cuda", sizes=SIZES, probs=cli_probs())
        cpu = run_cli(tmp_path, monkeypatch, "cpu" + tag, args, device="cpu", sizes=SIZES, probs=cli_probs())
        assert files(dev) == files(cpu)
        for f in files(cpu):
            if f.endswith(".csv") or "cell_territories" in f:
                assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f


def test_cli_nuclei_end_to_end_with_a_random_checkpoint(tmp_path, monkeypatch):
    """One --nuclei_dir run of the script with the network itself (random weights) on 3 synthetic 96 x 130 images: the CSVs of the
    device equal those of the script's CPU path."""
    import pandas as pd
    import quantify_droplets_batch as q
    from models.model_2 import UNetDC
    from tests.test_cells_cpu import write_masks
    from tests.test_tiling_cpu import write_images
    assert q.DEVICE == "cuda"
    monkeypatch.setattr(q, "IMG_SIZE", 64)
    sizes = ((96, 130),) * 3
    write_images(tmp_path / "imgs", sizes)
    write_masks(tmp_path / "nuc", sizes)
    torch.manual_seed(0)
    torch.save(UNetDC(3, 1).state_dict(), tmp_path / "m.pth")
    args = ["--img_dir", str(tmp_path / "imgs"), "--ckpt_path", str(tmp_path / "m.pth"), "--batch", "2", "--skip_excel",
            "--skip_histogram", "--background_radius", "15", "--nuclei_dir", str(tmp_path / "nuc"), "--cell_radius", "40"]
    dev = q.main(args + ["--out_dir", str(tmp_path / "dev")])
    monkeypatch.setattr(q, "DEVICE", "cpu")
    cpu = q.main(args + ["--out_dir", str(tmp_path / "cpu")])
    assert len(pd.read_csv(dev / "cells.csv")) == 9 and len(pd.read_csv(dev / "cells_per_image.csv")) == 3
    for f in CSVS + tuple(f"im{i}_droplets.csv" for i in range(3)):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    for i in range(3):
        assert (dev / "cell_territories" / f"im{i}_cells.png").read_bytes() == (cpu / "cell_territories" / f"im{i}_cells.png").read_bytes()
