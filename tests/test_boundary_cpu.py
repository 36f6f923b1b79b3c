"""CPU: the host path of the surface distances (utils/droplet_boundary.py) against the plain-loop restatement
(tests/boundary_ref.py) on the small inputs of the GPU list, against a sampled brute force at the larger ones, hand cases with
the integers written out, the derived columns, the argument checks of the C-ABI entry point, and the two entry points on
their CPU paths."""
import functools
import math

import numpy as np
import pandas as pd
import pytest

from tests import boundary_ref as ref
from tests.test_match_cpu import BIG_PAIRS, big_pair, cli_gt_masks, small_pairs, write_gt
from tests.test_split_cpu import files, run_cli
from utils import droplet_boundary as db

INF = 2147483647
RADII = (1, 3, 64)


def restated_names():
    """Every small pair with sides <= 65, all of 37 x 53, and the two named maps."""
    return sorted(n for n, (A, _, _, _) in small_pairs().items() if max(A.shape) <= 65 or n in ("checkerboard", "full_row"))


def sampled_names():
    return sorted(n for n in small_pairs() if n.startswith("276x408/"))


def tols_for(R):
    return sorted({t for t in (0, 1, 2, 3, R) if t <= R})


@functools.lru_cache(maxsize=None)
def restated_distances(name):
    A, ka, B, kb = small_pairs()[name]
    return ref.distances(A.tolist(), ka, B.tolist(), kb)


def assert_record_equal(got, want):
    assert got["hist"].dtype == got["dmax"].dtype == got["a"].dtype == got["b"].dtype == np.int64
    assert got["hist"].tolist() == want["hist"] and got["dmax"].tolist() == want["dmax"]
    assert got["a"].tolist() == want["a"] and got["b"].tolist() == want["b"]


@pytest.mark.parametrize("name", restated_names())
def test_host_path_equals_plain_loops(name):
    A, ka, B, kb = small_pairs()[name]
    for R in RADII:
        want = ref.record_ref(None, ka, None, kb, R, restated_distances(name))
        got = db.boundary_record_numpy(A, ka, B, kb, R)
        assert_record_equal(got, want)
        tols = tols_for(R)
        cols, rcols = db.boundary_columns(got["hist"], got["dmax"], R, tols), ref.columns_ref(want["hist"], want["dmax"], R, tols)
        assert cols == rcols and list(cols) == list(rcols), (R, cols, rcols)
        assert all(type(cols[q]) is int for q in ("bd_px_pred", "bd_px_gt", "n_far_pred", "n_far_gt"))
        assert all(type(v) is float for q, v in cols.items() if not q.startswith(("bd_px", "n_far")))
        for side in ("a", "b"):
            oc = db.object_columns(got[side])
            rows = ref.object_ref(want[side])
            assert oc["bd_px"].tolist() == [r[0] for r in rows]
            for q, j in (("bd_rms", 1), ("bd_max", 2)):
                assert [None if math.isnan(v) else v for v in oc[q].tolist()] == [r[j] for r in rows], (side, q)
        assert db.boundary_record_numpy(A, ka, B, kb, R, objects=False)["a"] is None


def boundary_by_shifts(L, k):
    """The boundary pixels once more, without padding: the frame, then every pixel that differs from a neighbour."""
    a = np.where((L >= 1) & (L <= k), L, 0)
    b = np.zeros(a.shape, bool)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
    dv, dh = a[1:] != a[:-1], a[:, 1:] != a[:, :-1]
    b[1:] |= dv
    b[:-1] |= dv
    b[:, 1:] |= dh
    b[:, :-1] |= dh
    return b & (a >= 1)


def sampled_brute_force(A, ka, B, kb, seed):
    """200 boundary pixels per direction: their d2 by a vectorised brute force over ALL boundary pixels of the other map."""
    rng = np.random.default_rng(seed)
    ba, bb = boundary_by_shifts(A, ka), boundary_by_shifts(B, kb)
    assert np.array_equal(ba, db.boundary_mask(A, ka)) and np.array_equal(bb, db.boundary_mask(B, kb))
    out = []
    for mine, other in ((ba, bb), (bb, ba)):
        p, q = np.argwhere(mine).astype(np.int64), np.argwhere(other).astype(np.int64)
        pick = p[rng.choice(len(p), size=min(200, len(p)), replace=False)] if len(p) else p
        d2 = [int(((q - s) ** 2).sum(1).min()) if len(q) else INF for s in pick]
        out.append((pick, d2))
    return out


def d2_planes(A, ka, B, kb):
    ba, bb = db.boundary_mask(A, ka), db.boundary_mask(B, kb)
    return db._d2_to(bb), db._d2_to(ba)


@pytest.mark.parametrize("name", sampled_names() + sorted(BIG_PAIRS))
def test_host_path_equals_sampled_brute_force(name):
    A, ka, B, kb = big_pair(name) if name in BIG_PAIRS else small_pairs()[name]
    planes = d2_planes(A, ka, B, kb)
    for (pick, d2), plane in zip(sampled_brute_force(A, ka, B, kb, seed=5), planes):
        assert [int(plane[y, x]) for y, x in pick] == d2
    got = db.boundary_record_numpy(A, ka, B, kb, 64)
    n, far, top = got["hist"].sum(1).tolist(), got["hist"][:, -1].tolist(), int(got["dmax"].max())
    assert got["a"][0].sum() == n[0] and got["b"][0].sum() == n[1]
    if name == "noise9_vs_shifted":
        assert (n, sum(far), top) == ([71375, 71216], 0, 289)
    elif name == "one_vs_noise21":
        assert (n, sum(far), top) == ([4852, 127984], 100482, 269361)
        assert got["a"].tolist() == [[4852], [int(got["dmax"][0])], [int(got["a"][2, 0])]] and got["a"][2, 0] > 0
    elif name == "one_vs_one":
        assert n == [4852, 4852] and got["hist"][:, 0].tolist() == n and top == 0


def test_anchors():
    A, ka, B, kb = small_pairs()["37x53/cc_vs_shifted"]
    got = db.boundary_record_numpy(A, ka, B, kb, 64)
    assert (got["hist"].sum(1).tolist(), got["hist"][:, -1].tolist(), int(got["dmax"].max())) == ([350, 335], [0, 0], 9)
    for name, (A, ka, B, kb) in small_pairs().items():
        if name.endswith("/vs_zeros"):
            got = db.boundary_record_numpy(A, ka, B, kb, 64)
            n = int(db.boundary_mask(A, ka).sum())
            assert got["hist"][0, -1] == n and got["hist"][0].sum() == n and got["hist"][1].sum() == 0
            assert got["dmax"].tolist() == [INF if n else -1, -1]
            assert got["a"][2].sum() == n * INF and (not n or db.boundary_columns(got["hist"], got["dmax"], 64)["hd"] == math.inf)
        if name.endswith("/self"):
            got = db.boundary_record_numpy(A, ka, B, kb, 64)
            assert got["hist"][:, 1:].sum() == 0 and got["dmax"].max() <= 0 and got["hist"][0, 0] == got["hist"][1, 0]


# ---- hand cases: the expected integers are written out ---------------------------------------------------------------------
def record(A, ka, B, kb, R):
    got = db.boundary_record_numpy(np.asarray(A, np.int32), ka, np.asarray(B, np.int32), kb, R)
    assert_record_equal(got, ref.record_ref(np.asarray(A).tolist(), ka, np.asarray(B).tolist(), kb, R))
    return got


def test_two_pixels_three_and_four_apart():
    A, B = np.zeros((6, 7), np.int32), np.zeros((6, 7), np.int32)
    A[1, 1], B[4, 5] = 1, 1
    r4, r5 = record(A, 1, B, 1, 4), record(A, 1, B, 1, 5)
    assert r4["hist"].shape == (2, 18) and r4["hist"][:, 17].tolist() == [1, 1] and r4["hist"].sum() == 2      # far
    assert r5["hist"].shape == (2, 27) and r5["hist"][:, 25].tolist() == [1, 1] and r5["hist"].sum() == 2      # bin 25
    for r in (r4, r5):
        assert r["dmax"].tolist() == [25, 25] and r["a"].tolist() == [[1], [25], [25]] and r["b"].tolist() == [[1], [25], [25]]
    c4, c5 = db.boundary_columns(r4["hist"], r4["dmax"], 4), db.boundary_columns(r5["hist"], r5["dmax"], 5)
    assert c4["hd"] == 5.0 and c4["hd95"] == 4.0 and c4["assd"] == 4.0 and c4["n_far_pred"] == c4["n_far_gt"] == 1   # "at least 4"
    assert c5["hd"] == 5.0 and c5["hd95"] == 5.0 and c5["assd"] == 5.0 and c5["n_far_pred"] == 0 and c5["nsd_3"] == 0.0


def test_block_against_the_same_block_cut_in_two():
    A, B = np.zeros((8, 10), np.int32), np.zeros((8, 10), np.int32)
    A[2:6, 2:8] = 1                                            # 4 x 6: a ring of 16, four inner pixels
    B[2:6, 2:5], B[2:6, 5:8] = 1, 2                            # two 4 x 3 blocks: rings of 10 each, the cut columns 4 and 5 included
    r = record(A, 1, B, 2, 3)
    assert r["hist"][0].tolist() == [16] + [0] * 10            # every boundary pixel of the whole block is one of the halves
    assert r["hist"][1].tolist() == [16, 4] + [0] * 9          # the four inner cut pixels are boundary on the split side only
    assert r["dmax"].tolist() == [0, 1]
    assert r["a"].tolist() == [[16], [0], [0]] and r["b"].tolist() == [[10, 10], [1, 1], [2, 2]]
    c = db.boundary_columns(r["hist"], r["dmax"], 3, (0, 1))
    assert c["bprec_0"] == 1.0 and c["brec_0"] == 16 / 20 and c["nsd_0"] == 32 / 36 and c["nsd_1"] == 1.0 and c["hd"] == 1.0
    assert c["bf_0"] == 2 * 16 * 16 / (16 * 20 + 16 * 16)


def test_square_inside_a_concentric_square():
    A, B = np.zeros((9, 9), np.int32), np.zeros((9, 9), np.int32)
    A[3:6, 3:6], B[1:8, 1:8] = 1, 1                            # 3 x 3: ring of 8; 7 x 7: ring of 24
    r = record(A, 1, B, 1, 2)
    assert r["hist"][0].tolist() == [0, 0, 0, 0, 8, 0]         # every ring pixel of the small square is 2 from the large ring
    # large ring against the small ring: the corners are (2, 2) away (8 -> far), their neighbours (2, 1) (5 -> far), the twelve
    # pixels facing the small square 2 (bin 4)
    assert r["hist"][1].tolist() == [0, 0, 0, 0, 12, 12]
    assert r["dmax"].tolist() == [4, 8] and r["a"].tolist() == [[8], [4], [32]] and r["b"].tolist() == [[24], [8], [4 * 8 + 8 * 5 + 12 * 4]]
    oc = db.object_columns(r["b"])
    assert oc["bd_px"].tolist() == [24] and oc["bd_max"].tolist() == [math.sqrt(8)] and oc["bd_rms"].tolist() == [math.sqrt(120 / 24)]


def test_the_frame_counts_and_labels_above_max_are_background():
    full = np.ones((5, 6), np.int32)
    assert int(db.boundary_mask(full, 1).sum()) == 2 * 6 + 2 * 3 and not db.boundary_mask(full, 1)[1:4, 1:5].any()
    r = record(full, 1, full, 1, 1)
    assert r["hist"].tolist() == [[18, 0, 0], [18, 0, 0]] and r["a"].tolist() == [[18], [0], [0]]
    L = np.ones((5, 7), np.int32)
    L[2, 3] = 9                                                # above max: background, and its four neighbours become boundary
    b = db.boundary_mask(L, 1)
    assert int(b.sum()) == 20 + 4 and not b[2, 3] and b[1, 3] and b[3, 3] and b[2, 2] and b[2, 4]
    assert int(db.boundary_mask(L, 9).sum()) == 20 + 4 + 1     # within max it is an object of its own
    r = record(L, 1, np.ones((5, 7), np.int32), 1, 2)
    # against the frame of the full map: (1, 3) and (3, 3) are one row from it, (2, 2) and (2, 4) two rows and two columns
    assert r["hist"][0].tolist() == [20, 2, 0, 0, 2, 0] and r["hist"][1].tolist() == [20, 0, 0, 0, 0, 0]
    neg = L.copy()
    neg[2, 3] = -4
    assert np.array_equal(db.boundary_mask(neg, 1), b)


def test_adding_and_pooling():
    p = small_pairs()
    one, two = p["37x53/cc_vs_shifted"], p["7x65/split_vs_cc"]
    r1, r2 = db.boundary_record_numpy(*one, 3), db.boundary_record_numpy(*two, 3)
    pooled = db.pooled_row([(r1["hist"], r1["dmax"]), (r2["hist"], r2["dmax"])], 3)
    assert pooled == db.summary_row("ALL", r1["hist"] + r2["hist"], np.maximum(r1["dmax"], r2["dmax"]), 3)
    assert list(pooled) == db.column_names() and pooled["bd_px_pred"] == int(r1["hist"][0].sum() + r2["hist"][0].sum())
    rows = [db.summary_row("x", r["hist"], r["dmax"], 3) for r in (r1, r2)]
    assert pooled["nsd_1"] != (rows[0]["nsd_1"] + rows[1]["nsd_1"]) / 2           # the sums, not the mean of the ratios
    c0 = int(r1["hist"][:, :2].sum() + r2["hist"][:, :2].sum())
    assert pooled["nsd_1"] == c0 / (pooled["bd_px_pred"] + pooled["bd_px_gt"])
    assert pooled["hd"] == max(rows[0]["hd"], rows[1]["hd"])


def hist_of(R, row0, row1=None):
    h = np.zeros((2, R * R + 2), np.int64)
    for d, row in enumerate((row0, row1 or {})):
        for l, v in row.items():
            h[d, l] = v
    return h


def test_columns_percentile_ranks():
    R = 3
    # n = 1: rank 1; n = 20: rank 19; n = 21: rank ceil(19.95) = 20; n = 100: rank 95
    assert db.boundary_columns(hist_of(R, {4: 1}), [4, -1], R)["hd95"] == 2.0
    assert db.boundary_columns(hist_of(R, {0: 18, 1: 1, 9: 1}), [9, -1], R)["hd95"] == 1.0          # the 19th of 20
    assert db.boundary_columns(hist_of(R, {0: 18, 9: 2}), [9, -1], R)["hd95"] == 3.0
    assert db.boundary_columns(hist_of(R, {0: 19, 1: 1, 9: 1}), [9, -1], R)["hd95"] == 1.0          # the 20th of 21
    assert db.boundary_columns(hist_of(R, {0: 19, 9: 2}), [9, -1], R)["hd95"] == 3.0
    assert db.boundary_columns(hist_of(R, {0: 94, 4: 1, 9: 5}), [9, -1], R)["hd95"] == 2.0          # the 95th of 100
    assert db.boundary_columns(hist_of(R, {0: 94, 9: 6}), [9, -1], R)["hd95"] == 3.0
    assert db.boundary_columns(hist_of(R, {0: 95, 10: 5}), [50, -1], R)["hd95"] == 0.0
    c = db.boundary_columns(hist_of(R, {0: 90, 10: 10}), [50, -1], R)                                # far: "at least R"
    assert c["hd95"] == 3.0 and c["n_far_pred"] == 10 and c["hd"] == math.sqrt(50) and c["assd"] == 10 * 3.0 / 100
    assert db.boundary_columns(hist_of(R, {0: 100}, {4: 1}), [0, 4], R)["hd95"] == 2.0               # the larger direction


def test_columns_tolerances_and_empty_conventions():
    R = 3
    h = hist_of(R, {0: 2, 1: 3, 9: 4, 10: 1}, {0: 1, 5: 4})
    c = db.boundary_columns(h, [12, 5], R, (0, 3))
    assert (c["bprec_0"], c["brec_0"], c["nsd_0"]) == (2 / 10, 1 / 5, 3 / 15)
    assert (c["bprec_3"], c["brec_3"], c["nsd_3"]) == (9 / 10, 5 / 5, 14 / 15)          # tau = R: everything but the far bin
    assert c["bf_3"] == 2 * 9 * 5 / (9 * 5 + 5 * 10) and c["bf_0"] == 2 * 2 * 1 / (2 * 5 + 1 * 10)
    assert c["assd"] == math.fsum([3 * 1.0, 4 * 3.0, 1 * 3.0, 4 * math.sqrt(5)]) / 15
    with pytest.raises(ValueError):
        db.boundary_columns(h, [12, 5], R, (4,))
    with pytest.raises(ValueError):
        db.boundary_columns(h, [12, 5], R, (-1,))
    empty = db.boundary_columns(hist_of(R, {}), [-1, -1], R)
    assert [empty[q] for q in ("hd", "hd95", "assd")] == [0.0, 0.0, 0.0]
    assert all(empty[f"{q}_{t}"] == 1.0 for q in ("bprec", "brec", "bf", "nsd") for t in (1, 2, 3))
    half = db.boundary_columns(hist_of(R, {10: 7}), [INF, -1], R)                        # a prediction, no annotation
    assert half["hd"] == math.inf and half["hd95"] == 3.0 and half["assd"] == 3.0 and half["n_far_pred"] == 7
    assert all(half[f"{q}_{t}"] == 0.0 for q in ("bprec", "brec", "bf", "nsd") for t in (1, 2, 3))
    oc = db.object_columns(np.array([[2, 0, 3], [INF, -1, 4], [2 * INF, 0, 9]], np.int64))
    assert oc["bd_px"].tolist() == [2, 0, 3] and oc["bd_rms"][0] == oc["bd_max"][0] == math.inf
    assert math.isnan(oc["bd_rms"][1]) and math.isnan(oc["bd_max"][1]) and (oc["bd_rms"][2], oc["bd_max"][2]) == (math.sqrt(3.0), 2.0)


# ---- the C ABI, host only --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_boundary_abi_rejects_bad_arguments(lib):
    import ctypes
    from tests.test_abi_symbols import IMAGE_SIZES
    for h, w in IMAGE_SIZES:
        assert lib.unetdc_boundary_distances_workspace(h, w) == 10 * h * w + 64
    for h, w in ((0, 5), (5, 0), (-1, 5), (5, -1), (16385, 5), (5, 16385)):
        assert lib.unetdc_boundary_distances_workspace(h, w) == 0
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every check below fails before any HIP call

    def call(la=fake, lb=fake, ka=5, kb=5, h=64, w=64, R=5, ws=fake, bytes_=1 << 30, hist=fake, dmax=fake, oa=fake, ob=fake):
        return lib.unetdc_boundary_distances(la, ka, lb, kb, h, w, R, ws, bytes_, hist, dmax, oa, ob, None)
    for kw, msg in [(dict(la=None), b"null"), (dict(lb=None), b"null"), (dict(ws=None), b"null"), (dict(hist=None), b"null"),
                    (dict(dmax=None), b"null"), (dict(R=0), b"geometry"), (dict(R=65), b"geometry"), (dict(ka=-1), b"geometry"),
                    (dict(kb=-1), b"geometry"), (dict(h=0), b"geometry"), (dict(w=16385), b"geometry"),
                    (dict(ws=ctypes.c_void_p(4097)), b"aligned"), (dict(hist=ctypes.c_void_p(4100)), b"aligned")]:
        assert call(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    rc = call(bytes_=lib.unetdc_boundary_distances_workspace(64, 64) - 1)
    err = lib.unetdc_last_error()
    assert rc == -3 and err.startswith(b"boundary_distances") and b"workspace too small" in err, (rc, err)


# ---- the entry points on their CPU paths -----------------------------------------------------------------------------------
BD_COLUMNS = ["bd_px", "bd_rms", "bd_max"]


def test_cli_refuses_the_flags_without_their_partners(tmp_path, monkeypatch):
    gt_dir = write_gt(tmp_path / "gt", cli_gt_masks())
    for extra, word in ((["--boundary"], "--gt_dir"), (["--boundary_tol", "1,2"], "--boundary"),
                        (["--gt_dir", str(gt_dir), "--boundary", "2", "--boundary_tol", "1,3"], "0..2"),
                        (["--gt_dir", str(gt_dir), "--boundary", "65"], "1..64"), (["--gt_dir", str(gt_dir), "--boundary", "0"], "1..64")):
        with pytest.raises(SystemExit, match=word):
            run_cli(tmp_path, monkeypatch, "refused", extra)
    assert not (tmp_path / "refused").exists()


def test_cli_boundary_on_the_cpu_path(tmp_path, monkeypatch):
    from tests.test_match_cpu import GT_COLUMNS, MATCH_COLUMNS
    from tests.test_shape_cpu import cc_labels
    from tests.test_split_cpu import cli_probs
    gts = cli_gt_masks()
    gt_dir = write_gt(tmp_path / "gt", gts)
    base = ["--gt_dir", str(gt_dir)]
    plain = run_cli(tmp_path, monkeypatch, "plain", base)
    out = run_cli(tmp_path, monkeypatch, "scored", base + ["--boundary", "8", "--boundary_tol", "0,2"])
    assert sorted(set(files(out)) - set(files(plain))) == ["boundary_per_image.csv"]
    per_image = pd.read_csv(out / "boundary_per_image.csv", float_precision="round_trip")
    assert list(per_image.columns) == db.column_names((0, 2)) and per_image["filename"].tolist() == ["im0.png", "im1.png", "im2.png", "ALL"]
    gt_all = pd.read_csv(out / "gt_droplets.csv", float_precision="round_trip")
    assert list(gt_all.columns) == GT_COLUMNS + BD_COLUMNS
    old_gt = pd.read_csv(plain / "gt_droplets.csv", float_precision="round_trip")
    assert gt_all[GT_COLUMNS].equals(old_gt)
    recs = []
    for i in range(3):
        A, B = cc_labels((cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8)), cc_labels(gts[i])
        ka, kb = int(A.max(initial=0)), int(B.max(initial=0))
        want = ref.record_ref(A.tolist(), ka, B.tolist(), kb, 8)
        recs.append(want)
        row = per_image.iloc[i].to_dict()
        assert {q: (int(v) if q.startswith(("bd_px", "n_far")) else float(v)) for q, v in row.items() if q != "filename"} == \
            ref.columns_ref(want["hist"], want["dmax"], 8, (0, 2))
        if ka:
            got = pd.read_csv(out / f"im{i}_droplets.csv", float_precision="round_trip")
            old = pd.read_csv(plain / f"im{i}_droplets.csv", float_precision="round_trip")
            assert list(got.columns) == list(old.columns) + BD_COLUMNS and got[list(old.columns)].equals(old)
            assert list(old.columns)[-3:] == MATCH_COLUMNS
            assert list(zip(*(got[q].tolist() for q in BD_COLUMNS))) == ref.object_ref(want["a"])
        rows = gt_all[gt_all["filename"] == f"im{i}.png"]
        assert list(zip(*(rows[q].tolist() for q in BD_COLUMNS))) == ref.object_ref(want["b"])
    hist = [[sum(r["hist"][d][l] for r in recs) for l in range(66)] for d in (0, 1)]
    dmax = [max(r["dmax"][d] for r in recs) for d in (0, 1)]
    allrow = per_image.iloc[3].to_dict()
    assert {q: (int(v) if q.startswith(("bd_px", "n_far")) else float(v)) for q, v in allrow.items() if q != "filename"} == \
        ref.columns_ref(hist, dmax, 8, (0, 2))
    assert per_image["hd"][2] == math.inf and per_image["bd_px_pred"][2] == 0 and per_image["bd_px_gt"][2] == 36   # nothing predicted
    assert 0 < per_image["hd"][1] < 3 and per_image["nsd_2"][1] > 0.9                    # the noise moved by one pixel
    for f in files(plain):                                         # everything else: byte for byte
        if f not in {"all_droplets.csv", "gt_droplets.csv"} | {f"im{i}_droplets.csv" for i in range(3)}:
            assert (out / f).read_bytes() == (plain / f).read_bytes(), f


def test_train_reports_the_boundary_keys(tmp_path, capsys):
    import train_DC_focal as t
    from tests.test_sweep_cpu import TRAIN_ARGS
    ck = str(tmp_path / "ck.pth")
    h = t.main(TRAIN_ARGS + ["--ckpt_path", ck, "--boundary"])
    b = h.test["boundary"]
    assert b["R"] == 64 and b["hist"].shape == (2, 64 * 64 + 2) and b["hist"].dtype == np.int64 and b["dmax"].shape == (2,)
    assert {"hd95", "assd", "nsd_1", "nsd_2", "nsd_3", "bf_1", "bf_2", "bf_3", "hd", "bd_px_pred", "bd_px_gt"} <= set(b)
    assert b["bd_px_gt"] == int(b["hist"][1].sum()) > 0
    assert "Boundary (--boundary 64, pooled): HD95" in capsys.readouterr().out
    plain = t.main(TRAIN_ARGS + ["--ckpt_path", ck])
    assert "boundary" not in plain.test
    assert t.build_parser().parse_args(["--boundary", "7"]).boundary == 7
    with pytest.raises(SystemExit):
        t.main(TRAIN_ARGS + ["--ckpt_path", ck, "--boundary", "65"])
