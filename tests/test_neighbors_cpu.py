"""CPU: droplet neighbourhoods.  utils/droplet_neighbors.py against the all-pixel-pairs brute force of
tests/neighbors_ref.py on the hand fixtures, the edge geometries and random maps; the host-only part of the C ABI; the record;
quantify_droplets_batch.py --neighbors on the CPU path.  Integer work: every comparison is exact."""
import ctypes
import dataclasses

import numpy as np
import pandas as pd
import pytest
import torch

from tests import neighbors_ref as ref
from utils import droplet_neighbors as dn

RADII = (1, 2, 5, 32)


def host_pairs(lab, k, G):
    return list(zip(*(v.tolist() for v in dn.neighbor_pairs_numpy(lab, k, G))))


def assert_equals_brute_force(lab, k, G):
    want = ref.brute_pairs(lab, k, G)
    rec = dn.neighbors_numpy(lab, k, G)
    got = list(zip(*(rec["pairs"][q].tolist() for q in ("a", "b", "d2"))))
    assert got == want, (G, got[:5], want[:5])
    cols = ref.brute_columns(np.where((np.asarray(lab) >= 1) & (np.asarray(lab) <= k), lab, 0), k, want)
    for q in dn.COLUMN_NAMES:
        assert rec[q].dtype == np.int64 and rec[q].tolist() == cols[q], (q, G)
    return want


@pytest.mark.parametrize("name", sorted(ref.hand_fixtures()))
def test_hand_fixtures(name):
    lab, k, G, want = ref.hand_fixtures()[name]
    assert ref.brute_pairs(lab, k, G) == want                  # the answers written out by hand are the definition's
    assert assert_equals_brute_force(lab, k, G) == want


def test_hand_fixtures_say_what_they_are_meant_to():
    fx = ref.hand_fixtures()
    lab, k, G, _ = fx["disc_not_square"]
    far = dict(((a, b), d) for a, b, d in ref.brute_pairs(lab, k, 6))
    assert far[(1, 2)] == 32 and far[(1, 4)] == 36             # inside the square window of G = 5, outside its disc
    lab, k, G, pairs = fx["behind_in_column"]
    rec = dn.neighbors_numpy(lab, k, G)
    assert rec["degree"].tolist() == [2, 2, 2] and rec["cluster"].tolist() == [1, 1, 1] and rec["cluster_size"].tolist() == [3, 3, 3]
    assert rec["nn_label"].tolist() == [2, 1, 2] and rec["nn_d2"].tolist() == [9, 9, 9]       # the tie at 9 goes to the smaller label
    lab, k, G, pairs = fx["chain_and_islands"]
    rec = dn.neighbors_numpy(lab, k, G)
    assert rec["cluster"].tolist() == [1, 1, 1, 1, 5, 5, 7] and rec["cluster_size"].tolist() == [4, 4, 4, 4, 2, 2, 1]
    assert rec["degree"].tolist() == [1, 2, 2, 1, 1, 1, 0]
    assert rec["nn_label"][6] == 0 and rec["nn_d2"][6] == dn.EDT_INF == ref.INF
    s = dn.summary(tuple(rec["pairs"][q] for q in ("a", "b", "d2")), rec)
    assert s == {"n_contacts": 4, "n_clusters": 2, "n_clustered": 6, "n_isolated": 1, "largest_cluster": 4,
                 "mean_nn_dist_px": (4 * 3.0 + 2 * 2.0) / 6, "n_touching": 0}


@pytest.mark.parametrize("name", sorted(ref.edge_maps()))
def test_edge_geometries(name):
    lab, k = ref.edge_maps()[name]
    for G in (1, 2, 5, 64):
        pairs = assert_equals_brute_force(lab, k, G)
        assert all(1 <= a < b <= k for a, b, _ in pairs)
    if name in ("1x1", "1x1_empty", "empty", "one_droplet_fills_the_image", "max_label_0"):
        assert host_pairs(lab, k, 64) == []
    if name == "label_without_pixel":
        rec = dn.neighbors_numpy(lab, k, 2)
        assert rec["cluster_size"].tolist() == [0, 2, 0, 2, 0] and rec["cluster"].tolist() == [1, 2, 3, 2, 5]
        assert rec["nn_label"].tolist() == [0, 4, 0, 2, 0] and rec["degree"].tolist() == [0, 1, 0, 1, 0]
    if name == "labels_above_max_label":
        assert host_pairs(lab, k, 2) == [(1, 2, 4)] and host_pairs(lab, 4, 2) == [(1, 2, 4), (2, 3, 4), (3, 4, 4)]


@pytest.mark.parametrize("G", RADII)
def test_random_maps_equal_the_brute_force(G):
    lab, n = ref.random_map()
    assert lab.shape == (70, 150) and n > 50
    pairs = assert_equals_brute_force(lab, n, G)
    assert len(pairs) == len(ref.brute_pairs(lab, n, G)) and (G < 5 or len(pairs) > n // 2)
    assert_equals_brute_force(lab, n // 2, G)                  # half the labels are background
    if G <= 5:
        tlab, tk = ref.touching_map()
        tp = assert_equals_brute_force(tlab, tk, G)
        assert sum(1 for _, _, d in tp if d == 1) > 20


def arrays_equal(x, y):
    return len(x) == len(y) and all(u.dtype == np.int64 and np.array_equal(u, v) for u, v in zip(x, y))


def test_offset_pairs_equal_the_brute_force_and_the_host_path():
    """The plain reference of the long-list GPU tests, on maps of single-pixel droplets small enough for the brute force."""
    for (h, w, step), radii in (((9, 11, 1), (1, 2, 3)), ((12, 13, 2), (2, 3, 5)), ((10, 14, 3), (3, 5, 9)), ((1, 9, 1), (1, 4))):
        lab, k = ref.lattice_map(h, w, step, seed=h)
        assert np.array_equal(np.sort(lab[lab > 0]), np.arange(1, k + 1)) and (lab[::step, ::step] > 0).all()
        for G in radii:
            for kk in (k, k // 2, 0):
                got = ref.offset_pairs(lab, kk, G)
                assert list(zip(*(v.tolist() for v in got))) == ref.brute_pairs(lab, kk, G), (h, w, step, G, kk)
                assert arrays_equal(got, dn.neighbor_pairs_numpy(lab, kk, G))
    lab, k, G, want = ref.hand_fixtures()["chain_and_islands"]
    assert list(zip(*(v.tolist() for v in ref.offset_pairs(lab, k, G)))) == want
    messy, k = ref.edge_maps()["out_of_range_values"]
    assert arrays_equal(ref.offset_pairs(messy, k, 2), dn.neighbor_pairs_numpy(messy, k, 2))


@pytest.mark.parametrize("lattice", ref.LATTICES, ids=lambda v: "{}x{}_step{}_G{}".format(*v[:4]))
def test_lattices_pass_the_sort_chunks_they_are_for(lattice):
    h, w, step, G, k, n = lattice
    lab, got_k = ref.lattice_map(h, w, step)
    assert got_k == k > 4096 and np.array_equal(np.sort(lab[lab > 0]), np.arange(1, k + 1))
    assert not np.array_equal(lab[lab > 0], np.arange(1, k + 1))                  # label order is not raster order
    pairs = ref.offset_pairs(lab, k, G)
    assert arrays_equal(pairs, dn.neighbor_pairs_numpy(lab, k, G)) and len(pairs[0]) == n
    assert {8191: 4096 < n < 8192, 8320: 8192 < n < 16384, 16512: 16384 < n, 48778: 2 * 16384 < n < 1 << 16}[n]
    cols = dn.neighbor_columns(pairs, k)
    assert (cols["nn_d2"] == step * step).all() and cols["degree"].min() >= 2     # every droplet has a partner at the lattice step
    a, b, d2 = pairs
    ties = np.bincount(np.concatenate([a, b])[np.concatenate([d2, d2]) == step * step], minlength=k + 1)[1:]
    assert ties.min() >= 2                                                         # ... at least two of them: the smaller label wins
    assert (cols["cluster"] == 1).all() and (cols["cluster_size"] == k).all()
    half = ref.offset_pairs(lab, k // 2, G)
    assert arrays_equal(half, dn.neighbor_pairs_numpy(lab, k // 2, G)) and 0 < len(half[0]) < n // 2
    assert len(np.unique(dn.neighbor_columns(half, k // 2, dn.present_labels(lab, k // 2))["cluster"])) > 1     # no longer one cluster


def test_the_cap_lattice_passes_the_grids_of_the_per_label_and_per_pair_kernels():
    h, w, step, G, k, n = ref.CAP_LATTICE
    lab, got_k = ref.lattice_map(h, w, step)
    a, b, d2 = ref.offset_pairs(lab, k, G)
    assert got_k == k > 2048 * 256 and len(a) == n > 2048 * 256 and n <= 1 << 21 and (d2 == 4).all()
    assert len(np.unique((a << 32) | b)) == n and (a < b).all()
    # the same pairs by position: each droplet with its right and its lower neighbour
    grid = lab[::step, ::step].astype(np.int64)
    by_hand = np.concatenate([(np.minimum(p, q) << 32 | np.maximum(p, q)).ravel()
                              for p, q in ((grid[:, :-1], grid[:, 1:]), (grid[:-1], grid[1:]))])
    assert np.array_equal(np.sort(by_hand), (a << 32) | b)


def test_patch_map_has_thousands_of_clusters_of_known_sizes():
    lab, K, cluster, size = ref.patch_map()
    G = ref.PATCH_G
    pairs = ref.offset_pairs(lab, K, G)
    assert arrays_equal(pairs, dn.neighbor_pairs_numpy(lab, K, G)) and len(pairs[0]) > 3 * 4096
    present = dn.present_labels(lab, K)
    assert (~present).sum() == ref.PATCH_MISSING and K > 4096
    cols = dn.neighbor_columns(pairs, K, present)
    assert np.array_equal(cols["cluster"], cluster) and np.array_equal(cols["cluster_size"], size)
    assert len(np.unique(cluster[present])) == (512 // 8) * (520 // 8) == 4160
    assert sorted(set(size.tolist())) == [0, 1, 2, 3, 4, 6, 9] and (size[~present] == 0).all()
    assert set(cols["degree"].tolist()) == {0, 1, 2, 3, 4} and (cols["nn_label"][size == 1] == 0).all()
    # no pair joins two patches: more than G pixels of background between any two
    fg = lab > 0
    assert not fg[5::8].any() and not fg[6::8].any() and not fg[7::8].any() and not fg[:, 5::8].any() and not fg[:, 6::8].any() and not fg[:, 7::8].any()


def test_check_radius_and_helpers():
    assert dn.check_radius(1) == 1 and dn.check_radius(np.int64(64)) == 64 and dn.DEFAULT_RADIUS == 5
    for bad in (0, 65, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            dn.check_radius(bad)
    empty = tuple(np.zeros(0, np.int64) for _ in range(3))
    cols = dn.neighbor_columns(empty, 0)
    assert all(cols[q].shape == (0,) for q in dn.COLUMN_NAMES)
    assert dn.summary(empty, cols)["n_isolated"] == 0 and np.isnan(dn.summary(empty, cols)["mean_nn_dist_px"])
    cols = dn.neighbor_columns(empty, 3)
    assert cols["cluster"].tolist() == [1, 2, 3] and cols["cluster_size"].tolist() == [1, 1, 1]
    t = dn.table_columns(dn.neighbors_numpy(ref.pixels(1, 9, (0, 0), (0, 3), (0, 8)), 3, 3), [0.0, 0.0, 0.0], [0.0, 3.0, 8.0], 2.0)
    assert t["nn_label"].tolist() == [2, 1, 0] and t["nn_dist_px"][:2].tolist() == [3.0, 3.0] and np.isnan(t["nn_dist_px"][2])
    assert t["nn_centroid_dist_px"][:2].tolist() == [3.0, 3.0] and t["nn_dist_micron"][:2].tolist() == [1.5, 1.5]


def test_record_fields_default_to_off_and_old_constructions_keep_their_meaning():
    from unet_dc_segmentation_amd._lib import UnetdcError
    from unet_dc_segmentation_amd.droplets import DropletOptions, Droplets
    o = DropletOptions(1.5, True, True, 0.4, -1)
    assert (o.split_depth, o.shape, o.labels, o.thresh_low, o.max_hole_area, o.neighbors) == (1.5, True, True, 0.4, -1, None)
    assert DropletOptions().neighbors is None and DropletOptions(neighbors=5).neighbors == 5
    assert [f.name for f in dataclasses.fields(DropletOptions)][:6] == ["split_depth", "shape", "labels", "thresh_low",
                                                                        "max_hole_area", "neighbors"]
    assert DropletOptions(labels=True, neighbors=3).labels             # the neighbour route has a label map
    for bad in (0, 65, 2.5, "5"):
        with pytest.raises(UnetdcError):
            DropletOptions(neighbors=bad)
    with pytest.raises(UnetdcError):
        dataclasses.replace(DropletOptions(), neighbors=100, thresh=0.5)
    d = Droplets(np.zeros((2, 2), np.uint8), np.zeros(0, np.int64), np.zeros(0), np.zeros(0), None, None, np.ones(4, np.int64))
    assert d.neighbors is None and d.clean_counts.tolist() == [1, 1, 1, 1]
    assert [f.name for f in dataclasses.fields(Droplets)][6:8] == ["clean_counts", "neighbors"]    # the positions they were given
    assert len(list(d)) == 4


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_abi_workspace_query(lib):
    assert lib.unetdc_version() == 2
    q = lib.unetdc_label_neighbors_workspace
    assert q(1, 1, 0, 0) > 0 and q(16384, 16384, 1 << 16, 1 << 20) > 0
    assert q(64, 64, 100, 10) >= 64 * 64 * 4 and q(64, 64, 100, 1000) > q(64, 64, 100, 10)
    assert q(64, 64, 100, 100 * 99 // 2) == q(64, 64, 100, 1 << 30)          # room beyond K (K - 1) / 2 pairs buys nothing
    assert q(64, 64, 100, 10) % 8 == 0
    for h, w, k, m in ((0, 8, 4, 4), (8, 0, 4, 4), (-1, 8, 4, 4), (16385, 8, 4, 4), (8, 16385, 4, 4), (8, 8, -1, 4), (8, 8, 4, -1)):
        assert q(h, w, k, m) == 0, (h, w, k, m)


def test_abi_refuses_before_any_hip_call(lib):
    """Null and range arguments come back as UNETDC_EINVAL (EWORKSPACE for a short workspace) with a message, before any HIP
    call: host memory stands in for the device pointers."""
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    a += (-a) % 16
    need = lib.unetdc_label_neighbors_workspace(8, 8, 4, 6)
    assert 0 < need < (1 << 16) - 16
    ok = dict(label=a, k=4, h=8, w=8, G=3, ws=a, nbytes=need, count=a, pa=a, pb=a, pd=a, m=6, nn=a, nd=a, deg=a, cl=a, cs=a)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.unetdc_label_neighbors(v["label"], v["k"], v["h"], v["w"], v["G"], v["ws"], v["nbytes"], v["count"], v["pa"],
                                          v["pb"], v["pd"], v["m"], v["nn"], v["nd"], v["deg"], v["cl"], v["cs"], None)

    for kw in (dict(label=None), dict(ws=None), dict(count=None), dict(pa=None), dict(pb=None), dict(pd=None), dict(nn=None),
               dict(nd=None), dict(deg=None), dict(cl=None), dict(cs=None)):
        assert call(**kw) == -1 and b"null" in lib.unetdc_last_error(), kw
    for kw in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385), dict(h=-3), dict(G=0), dict(G=65), dict(G=-1), dict(k=-1),
               dict(m=-1)):
        assert call(**kw) == -1 and b"geometry" in lib.unetdc_last_error(), kw
    assert call(ws=a + 4) == -1 and b"aligned" in lib.unetdc_last_error()
    assert call(nbytes=need - 1) == -3 and b"workspace too small" in lib.unetdc_last_error()
    assert call(nbytes=0) == -3


# ---- quantify_droplets_batch.py on the CPU path --------------------------------------------------------------------------
def cli_probs():
    """Three 64 x 64 maps: many small droplets, two discs two pixels apart, nothing."""
    from scipy import ndimage
    yy, xx = np.mgrid[0:64, 0:64]
    many = ndimage.binary_opening(np.random.default_rng(5).random((64, 64)) < 0.45)
    discs = ((yy - 32) ** 2 + (xx - 20) ** 2 <= 81) | ((yy - 32) ** 2 + (xx - 41) ** 2 <= 81)
    p = np.stack([np.where(many, 0.9, 0.1), np.where(discs, 0.9, 0.1), np.full((64, 64), 0.1)])
    return torch.from_numpy(p.astype(np.float32))[:, None]


def cli_masks():
    return [(cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8) for i in range(3)]


def test_cli_parser():
    import quantify_droplets_batch as q
    p = q.build_parser()
    assert p.parse_args(["--img_dir", "x"]).neighbors is None
    assert p.parse_args(["--img_dir", "x", "--neighbors"]).neighbors == 5
    assert p.parse_args(["--img_dir", "x", "--neighbors", "64"]).neighbors == 64
    for bad in ("0", "65", "-2", "2.5", "abc"):
        with pytest.raises(SystemExit) as e:
            p.parse_args(["--img_dir", "x", "--neighbors", bad])
        assert e.value.code == 2, bad                          # a parser error


@pytest.mark.parametrize("extra", [[], ["--px_per_micron", "2.0", "--min_area", "4"], ["--split_touching", "--split_depth", "1.0"],
                                   ["--droplet_shape"]])
def test_cli_on_the_cpu_path(tmp_path, monkeypatch, extra):
    import quantify_droplets_batch as q
    from tests.test_split_cpu import files, run_cli
    from utils.droplet_match import gt_labels_numpy
    G = 4
    off = run_cli(tmp_path, monkeypatch, "off", extra, probs=cli_probs())
    on = run_cli(tmp_path, monkeypatch, "on", extra + ["--neighbors", str(G)], probs=cli_probs())
    assert sorted(set(files(on)) - set(files(off))) == ["droplet_contacts.csv"]
    assert list(pd.read_csv(off / "summary_per_image.csv").columns) == ["filename", "droplet_count", "total_area_px"]
    old_columns = list(pd.read_csv(off / "all_droplets.csv").columns)
    assert not {"nn_label", "cluster", "n_contacts"} & set(old_columns)
    for f in files(off):                                       # the flag changes no mask and no label image
        if f.endswith(".png"):
            assert (off / f).read_bytes() == (on / f).read_bytes(), f
    min_area = 4 if "--min_area" in extra else 1
    split = "--split_touching" in extra
    new = ["nn_label", "nn_dist_px", "nn_centroid_dist_px", "n_contacts", "cluster", "cluster_size"]
    new += ["nn_dist_micron"] if "--px_per_micron" in extra else []
    contacts = pd.read_csv(on / "droplet_contacts.csv")
    assert list(contacts.columns) == ["filename", "label_a", "label_b", "d2", "dist_px"]
    summary = pd.read_csv(on / "summary_per_image.csv")
    assert list(summary.columns) == ["filename", "droplet_count", "total_area_px"] + list(dn.SUMMARY_NAMES)
    for i, m in enumerate(cli_masks()):
        if split:
            from utils.droplet_split import split_labels
            lab = split_labels(m, 2, min_area)[0]
        else:
            lab = gt_labels_numpy(m, min_area)
        k = int(lab.max())
        rec = dn.neighbors_numpy(lab, k, G)
        want = ref.brute_pairs(lab, k, G)
        rows = contacts[contacts["filename"] == f"im{i}.png"]
        assert list(zip(rows["label_a"].tolist(), rows["label_b"].tolist(), rows["d2"].tolist())) == want        # (a, b) order
        assert np.array_equal(rows["dist_px"].to_numpy(), np.sqrt(np.array([d for _, _, d in want], np.float64)))
        s = dn.summary(tuple(rec["pairs"][c] for c in ("a", "b", "d2")), rec)
        for name in dn.SUMMARY_NAMES:
            got = summary[name][i]
            assert (np.isnan(got) and np.isnan(s[name])) or got == s[name], (name, i)
        assert summary["droplet_count"][i] == k
        if k == 0:
            continue
        t = pd.read_csv(on / f"im{i}_droplets.csv", float_precision="round_trip")
        told = pd.read_csv(off / f"im{i}_droplets.csv", float_precision="round_trip")
        assert list(t.columns) == list(told.columns) + new     # behind the table's own, the shape and the micron columns
        assert t["area"].equals(told["area"]) and t["label"].tolist() == list(range(1, k + 1))
        cols = dn.table_columns(rec, t["centroid-0"].to_numpy(), t["centroid-1"].to_numpy(), 2.0 if "nn_dist_micron" in new else None)
        for name in new:
            assert np.array_equal(t[name].to_numpy(), cols[name], equal_nan=True), (name, i)
        assert t["n_contacts"].sum() == 2 * len(want)
    assert summary["n_contacts"][0] > 5 and summary["n_contacts"][2] == 0
    if split:
        assert summary["n_touching"][0] > 0                    # cut droplets touch: d2 = 1
    elif min_area == 1:
        assert summary["n_contacts"][1] == 1 and contacts[contacts["filename"] == "im1.png"]["d2"].tolist() == [9]


def test_cli_without_a_single_contact_still_writes_the_header(tmp_path, monkeypatch):
    from tests.test_split_cpu import run_cli
    p = cli_probs()
    p[0] = p[2]
    out = run_cli(tmp_path, monkeypatch, "on", ["--neighbors", "1"], probs=p)
    assert list(pd.read_csv(out / "droplet_contacts.csv").columns) == ["filename", "label_a", "label_b", "d2", "dist_px"]
    assert pd.read_csv(out / "summary_per_image.csv")["n_contacts"].tolist() == [0, 0, 0]
