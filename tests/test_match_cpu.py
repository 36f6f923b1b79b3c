"""CPU: the host path of the droplet matching (utils/droplet_match.py) against the plain-loop restatement
(tests/match_ref.py) on every input the GPU tests use, known answers, the pooled row, the argument checks of the new C-ABI
entry point, and quantify_droplets_batch.py --gt_dir on its CPU path."""
import functools

import numpy as np
import pandas as pd
import pytest
from PIL import Image

from tests.match_ref import match_ref, overlap_table_ref, ratios_ref
from tests.test_shape_cpu import cc_labels, split_labels
from tests.test_split_cpu import SIZE, cli_probs, files, noise_mask, run_cli
from utils import droplet_match as dm

FULL = (1040, 1388)


def shift(m, dy, dx):
    """m moved down by dy and right by dx, zeros moving in."""
    out = np.zeros_like(m)
    h, w = m.shape
    out[dy:, dx:] = m[:h - dy, :w - dx]
    return out


def kmax(lab):
    return int(lab.max(initial=0))


SMALL_SIDES = ((1, 1), (1, 65), (37, 53), (276, 408), (5, 63), (6, 64), (7, 65))


@functools.lru_cache(maxsize=None)
def small_pairs():
    """name -> (A, ka, B, kb): the small inputs of the GPU list."""
    out = {}
    for h, w in SMALL_SIDES:
        m = np.ones((1, 1), np.uint8) if (h, w) == (1, 1) else noise_mask(h, w, seed=h + w, sigma=2.0 if h > 1 else 0.0)
        cc, tag = cc_labels(m), f"{h}x{w}/"
        moved = cc_labels(shift(m, min(1, h - 1), min(2, w - 1)))
        out[tag + "cc_vs_shifted"] = (cc, kmax(cc), moved, kmax(moved))
        sp = split_labels(m)
        out[tag + "split_vs_cc"] = (sp, kmax(sp), cc, kmax(cc))
        out[tag + "self"] = (cc, kmax(cc), cc, kmax(cc))
        out[tag + "vs_zeros"] = (cc, kmax(cc), np.zeros((h, w), np.int32), 0)
        out[tag + "one_label_vs_cc"] = (np.ones((h, w), np.int32), 1, cc, kmax(cc))
    yy, xx = np.mgrid[0:21, 0:130]
    out["checkerboard"] = ((1 + (yy + xx) % 2).astype(np.int32), 2, (1 + xx % 3).astype(np.int32), 3)   # every lane a run head
    row = np.zeros((3, 1388), np.int32)
    row[1] = 1
    out["full_row"] = (row, 1, np.full((3, 1388), 2, np.int32), 2)                                       # a run longer than a wave
    return out


@functools.lru_cache(maxsize=None)
def big_labels(name):
    if name == "noise9":
        return cc_labels(noise_mask(*FULL, seed=9, sigma=6.0, frac=0.35))
    if name == "noise21":
        return cc_labels(noise_mask(*FULL, seed=21, sigma=3.0, frac=0.3))
    if name == "noise9_shifted":
        return cc_labels(shift(noise_mask(*FULL, seed=9, sigma=6.0, frac=0.35), 2, 1))
    assert name == "one"
    return np.ones(FULL, np.int32)


BIG_PAIRS = {"noise9_vs_noise21": ("noise9", "noise21"), "noise9_vs_shifted": ("noise9", "noise9_shifted"),
             "one_vs_noise21": ("one", "noise21"), "one_vs_one": ("one", "one")}


def big_pair(name):
    A, B = (big_labels(q) for q in BIG_PAIRS[name])
    return A, kmax(A), B, kmax(B)


def areas(lab, k):
    return np.bincount(lab.ravel(), minlength=k + 1)[1:k + 1].astype(np.int64)


def assert_equals_restatement(A, ka, B, kb):
    a, b, n = dm.overlap_table_numpy(A, B, ka, kb)
    ref = overlap_table_ref(A.tolist(), B.tolist(), ka, kb)
    assert a.dtype == b.dtype == n.dtype == np.int64
    assert list(zip(a.tolist(), b.tolist(), n.tolist())) == ref
    area_a, area_b = areas(A, ka), areas(B, kb)
    got = dm.match_columns(area_a, area_b, a, b, n)
    pred, gt, image = match_ref(area_a.tolist(), area_b.tolist(), ref)
    assert list(zip(*(got["pred"][q].tolist() for q in ("gt_label", "gt_iou", "gt_covered")))) == pred
    assert list(zip(*(got["gt"][q].tolist() for q in ("pred_label", "pred_iou", "pred_covered")))) == gt
    assert got["image"] == image and all(type(v) is int for v in got["image"].values())
    row = dm.summary_row("x", got["image"])
    for q, v in ratios_ref(image).items():
        assert row[q] == v and type(row[q]) is float, q
    return got, row


@pytest.mark.parametrize("name", sorted(small_pairs()))
def test_host_path_equals_plain_loops_on_small_inputs(name):
    assert_equals_restatement(*small_pairs()[name])


@pytest.mark.parametrize("name", sorted(BIG_PAIRS))
def test_host_path_equals_plain_loops_at_full_size(name):
    A, ka, B, kb = big_pair(name)
    got, row = assert_equals_restatement(A, ka, B, kb)
    a, b, n = dm.overlap_table_numpy(A, B, ka, kb)
    if name == "noise9_vs_noise21":
        assert (len(n), ka, kb, int(np.bincount(a).max())) == (1955, 553, 2537, 94)
    elif name == "noise9_vs_shifted":
        assert len(n) == 549 and [row[q] for q in dm.TP_NAMES] == [444, 420, 386, 340, 264, 205, 119, 17, 1, 0]
    elif name == "one_vs_noise21":
        assert len(n) == 2537 and a.tolist() == [1] * 2537 and b.tolist() == list(range(1, 2538))
    else:
        assert n.tolist() == [FULL[0] * FULL[1]]


def test_small_inputs_hold_what_they_are_for():
    p = small_pairs()
    a, b, n = dm.overlap_table_numpy(*p["276x408/split_vs_cc"][:1], p["276x408/split_vs_cc"][2], p["276x408/split_vs_cc"][1],
                                     p["276x408/split_vs_cc"][3])
    assert len(a) == p["276x408/split_vs_cc"][1] > p["276x408/split_vs_cc"][3]            # every split droplet in one component
    assert len(dm.overlap_table_numpy(*[p["checkerboard"][i] for i in (0, 2, 1, 3)])[0]) == 6
    assert dm.overlap_table_numpy(*[p["full_row"][i] for i in (0, 2, 1, 3)])[2].tolist() == [1388]
    assert len(dm.overlap_table_numpy(*[p["37x53/vs_zeros"][i] for i in (0, 2, 1, 3)])[0]) == 0


def columns(A, B):
    ka, kb = kmax(A), kmax(B)
    a, b, n = dm.overlap_table_numpy(A, B, ka, kb)
    got = dm.match_columns(areas(A, ka), areas(B, kb), a, b, n)
    return (a.tolist(), b.tolist(), n.tolist()), got, dm.summary_row("x", got["image"])


def test_identical_maps_match_at_every_threshold():
    lab = cc_labels(noise_mask(90, 120, seed=5))
    k = kmax(lab)
    _, got, row = columns(lab, lab)
    assert k > 5 and [row[q] for q in dm.TP_NAMES] == [k] * 10 and row["mean_ap"] == 1.0
    assert got["pred"]["gt_label"].tolist() == list(range(1, k + 1)) and got["pred"]["gt_iou"].tolist() == [1.0] * k
    assert row["n_merged"] == row["n_split"] == row["n_missed"] == row["n_spurious"] == 0 and row["pixel_dice"] == 1.0


def test_disjoint_maps():
    A, B = np.zeros((20, 30), np.int32), np.zeros((20, 30), np.int32)
    A[2:5, 2:5], A[10:12, 3:9], B[15:18, 20:25] = 1, 2, 1
    t, got, row = columns(A, B)
    assert t == ([], [], []) and row["n_spurious"] == 2 and row["n_missed"] == 1 and row["mean_ap"] == 0.0
    assert got["pred"]["gt_label"].tolist() == [0, 0] and got["pred"]["gt_iou"].tolist() == [0.0, 0.0]


def bar(x0):
    m = np.zeros((3, 12), np.int32)
    m[1, x0:x0 + 6] = 1
    return m


def test_iou_of_exactly_one_half_is_not_a_match():
    t, got, row = columns(bar(2), bar(4))
    assert t == ([1], [1], [4])                                # n = 4, U = 8
    assert [row[q] for q in dm.TP_NAMES] == [0] * 10 and got["pred"]["gt_label"].tolist() == [0]
    assert got["pred"]["gt_iou"].tolist() == [0.0] and got["pred"]["gt_covered"].tolist() == [1]       # 2 * 4 > 6


def test_bar_shifted_by_one_matches_up_to_seven_tenths():
    t, got, row = columns(bar(2), bar(3))
    assert t == ([1], [1], [5])                                # n = 5, U = 7: 100 > 7 k for k = 10..14
    assert [row[q] for q in dm.TP_NAMES] == [1] * 5 + [0] * 5
    assert got["pred"]["gt_iou"].tolist() == [5 / 7] and got["gt"]["pred_iou"].tolist() == [5 / 7]
    assert row["mean_ap"] == (1.0 + 1.0 + 1.0 + 1.0 + 1.0) / 10


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def test_one_prediction_over_two_annotated_discs_is_merged():
    A, B = np.zeros((40, 60), np.int32), np.zeros((40, 60), np.int32)
    A[8:32, 5:55] = 1
    B[disc(40, 60, 20, 18, 9)], B[disc(40, 60, 20, 42, 9)] = 1, 2
    _, got, row = columns(A, B)
    assert row["n_merged"] == 1 and row["n_split"] == 0 and got["pred"]["gt_covered"].tolist() == [2] and row["tp_50"] == 0


def test_one_annotated_disc_under_two_half_predictions_is_split():
    B = disc(40, 40, 20, 20, 12).astype(np.int32)
    A = B.copy()
    A[:, 20:] *= 2
    _, got, row = columns(A, B)
    assert row["n_split"] == 1 and row["n_merged"] == 0 and got["gt"]["pred_covered"].tolist() == [2]


def test_empty_maps_and_empty_prediction():
    z = np.zeros((9, 9), np.int32)
    _, _, row = columns(z, z)
    ratio_names = ["precision_50", "recall_50", "f1_50", "mean_ap", "pixel_dice", "pixel_iou"] + list(dm.AP_NAMES)
    assert [row[q] for q in ratio_names] == [1.0] * 16
    B = z.copy()
    B[2:5, 2:5] = 1
    _, _, row = columns(z, B)
    assert [row[q] for q in ratio_names] == [0.0] * 16 and row["n_missed"] == 1 and row["n_pred"] == 0


def test_pooled_row_is_the_row_of_the_integer_sums():
    a = columns(bar(2), bar(3))[1]["image"]
    lab = cc_labels(noise_mask(90, 120, seed=5))
    b = columns(lab, cc_labels(shift(noise_mask(90, 120, seed=5), 1, 1)))[1]["image"]
    pooled = dm.pooled_row([a, b])
    assert pooled == dm.summary_row("ALL", {q: a[q] + b[q] for q in dm.INTEGER_NAMES})
    assert pooled["filename"] == "ALL" and pooled["n_pred"] == 1 + kmax(lab)
    assert pooled["mean_ap"] == sum(pooled[t] / (pooled["n_pred"] + pooled["n_gt"] - pooled[t]) for t in dm.TP_NAMES) / 10
    assert list(pooled) == ["filename"] + list(dm.COUNT_NAMES) + ["precision_50", "recall_50", "f1_50"] + list(dm.AP_NAMES) + \
        ["mean_ap"] + list(dm.PIXEL_NAMES) + ["pixel_dice", "pixel_iou"]


def test_labels_out_of_range_are_skipped():
    A, ka, B, kb = small_pairs()["37x53/cc_vs_shifted"]
    assert ka > 3 and kb > 3
    A2 = A.copy()
    A2[0, 0] = -7
    got = dm.overlap_table_numpy(A2, B, ka - 2, kb - 1)
    assert list(zip(*(v.tolist() for v in got))) == overlap_table_ref(A2.tolist(), B.tolist(), ka - 2, kb - 1)
    assert got[0].max() <= ka - 2 and got[1].max() <= kb - 1


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_match_abi_rejects_bad_arguments(lib):
    import ctypes
    assert lib.unetdc_label_overlap_workspace(1040, 1388, 1000) > 0
    assert lib.unetdc_label_overlap_workspace(1040, 1388, 0) > 0
    assert lib.unetdc_label_overlap_workspace(1040, 1388, 1 << 30) == lib.unetdc_label_overlap_workspace(1040, 1388, 1040 * 1388)
    assert lib.unetdc_label_overlap_workspace(0, 1388, 10) == 0 and lib.unetdc_label_overlap_workspace(8, 8, -1) == 0
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every check below fails before any HIP call

    def overlap(la=fake, lb=fake, ka=5, kb=5, h=64, w=64, ws=fake, bytes_=1 << 30, count=fake, out=fake, max_pairs=10):
        return lib.unetdc_label_overlap(la, ka, lb, kb, h, w, ws, bytes_, count, out, out, out, max_pairs, None)
    for kw, msg in [(dict(la=None), b"null"), (dict(lb=None), b"null"), (dict(ws=None), b"null"), (dict(count=None), b"null"),
                    (dict(out=None), b"null"), (dict(h=0), b"geometry"), (dict(w=16385), b"geometry"), (dict(ka=-1), b"geometry"),
                    (dict(kb=-1), b"geometry"), (dict(max_pairs=-1), b"geometry")]:
        assert overlap(**kw) == -1 and msg in lib.unetdc_last_error(), (kw, lib.unetdc_last_error())
    assert overlap(bytes_=lib.unetdc_label_overlap_workspace(64, 64, 10) - 1) == -3 and b"workspace" in lib.unetdc_last_error()
    assert lib.unetdc_version() == 2


# ---- quantify_droplets_batch.py --gt_dir on the CPU path -------------------------------------------------------------------
MATCH_COLUMNS = ["gt_label", "gt_iou", "gt_covered"]
GT_COLUMNS = ["filename", "label", "area", "centroid-0", "centroid-1", "pred_label", "pred_iou", "pred_covered"]


def cli_gt_masks():
    """Annotations for the three images of cli_probs: its two discs apart, the noise moved by a pixel, and one square where
    nothing is predicted."""
    masks = [(cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8) for i in range(3)]
    two = (disc(SIZE, SIZE, 32, 19, 11) | disc(SIZE, SIZE, 32, 44, 11)).astype(np.uint8)
    sq = np.zeros((SIZE, SIZE), np.uint8)
    sq[10:20, 10:20] = 1
    return [two, shift(masks[1], 1, 0), sq]


def write_gt(d, masks, scale=255):
    d.mkdir()
    for i, m in enumerate(masks):
        Image.fromarray((m * scale).astype(np.uint8)).save(d / f"im{i}.png")
    return d


@pytest.mark.parametrize("extra", [[], ["--split_touching"], ["--droplet_shape", "--density_maps"]])
def test_cli_gt_dir_on_the_cpu_path(tmp_path, monkeypatch, extra):
    gts = cli_gt_masks()
    gt_dir = write_gt(tmp_path / "gt", gts, scale=200)             # any nonzero grey is annotation
    plain = run_cli(tmp_path, monkeypatch, "plain", extra)
    out = run_cli(tmp_path, monkeypatch, "scored", extra + ["--gt_dir", str(gt_dir)])
    assert sorted(set(files(out)) - set(files(plain))) == ["gt_droplets.csv", "match_per_image.csv"]
    tables = {"all_droplets.csv"} | {f"im{i}_droplets.csv" for i in range(3)}
    for f in files(plain):                                         # everything but the droplet tables: byte for byte
        if f not in tables:
            assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    gt_all = pd.read_csv(out / "gt_droplets.csv", float_precision="round_trip")
    per_image = pd.read_csv(out / "match_per_image.csv", float_precision="round_trip")
    assert list(gt_all.columns) == GT_COLUMNS and per_image["filename"].tolist() == ["im0.png", "im1.png", "im2.png", "ALL"]
    images = []
    for i in range(3):
        m = (cli_probs()[i, 0].numpy() > 0.5).astype(np.uint8)
        A = split_labels(m) if "--split_touching" in extra else cc_labels(m)
        B = cc_labels(gts[i])
        ka, kb = kmax(A), kmax(B)
        ref = overlap_table_ref(A.tolist(), B.tolist(), ka, kb)
        pred, gt, image = match_ref(areas(A, ka).tolist(), areas(B, kb).tolist(), ref)
        images.append(image)
        if ka:
            got = pd.read_csv(out / f"im{i}_droplets.csv", float_precision="round_trip")
            old = pd.read_csv(plain / f"im{i}_droplets.csv", float_precision="round_trip")
            assert list(got.columns) == list(old.columns) + MATCH_COLUMNS and got[list(old.columns)].equals(old)
            assert list(zip(*(got[q].tolist() for q in MATCH_COLUMNS))) == pred
        rows = gt_all[gt_all["filename"] == f"im{i}.png"]
        assert rows["label"].tolist() == list(range(1, kb + 1)) and rows["area"].tolist() == areas(B, kb).tolist()
        assert list(zip(*(rows[q].tolist() for q in GT_COLUMNS[5:]))) == gt
        ys, xs = np.nonzero(B == 1)
        assert rows["centroid-0"].iloc[0] == ys.sum() / len(ys) and rows["centroid-1"].iloc[0] == xs.sum() / len(xs)
        r = per_image.iloc[i]
        assert {q: int(r[q]) for q in dm.INTEGER_NAMES} == image
        assert {q: float(r[q]) for q in ratios_ref(image)} == ratios_ref(image)
    pooled = {q: sum(im[q] for im in images) for q in dm.INTEGER_NAMES}
    r = per_image.iloc[3]
    assert {q: int(r[q]) for q in dm.INTEGER_NAMES} == pooled and {q: float(r[q]) for q in ratios_ref(pooled)} == ratios_ref(pooled)
    # image 0: the two predicted discs overlap into one component -- merged; cut by --split_touching they match one to one
    if "--split_touching" in extra:
        assert images[0]["n_merged"] == 0 and images[0]["tp_50"] == 2
    else:
        assert images[0]["n_merged"] == 1 and images[0]["tp_50"] == 0
    assert images[2]["n_pred"] == 0 and images[2]["n_missed"] == 1 and per_image["mean_ap"][2] == 0.0


def test_cli_gt_labels_and_min_area(tmp_path, monkeypatch):
    """A run scored against its own label images agrees with itself; --gt_min_area drops small annotated objects."""
    first = run_cli(tmp_path, monkeypatch, "first", ["--split_touching"])
    lab_dir = tmp_path / "labels"
    lab_dir.mkdir()
    for i in range(3):
        (lab_dir / f"im{i}.png").write_bytes((first / "predicted_masks" / f"im{i}_labels.png").read_bytes())
    again = run_cli(tmp_path, monkeypatch, "again", ["--split_touching", "--gt_dir", str(lab_dir), "--gt_labels"])
    per_image = pd.read_csv(again / "match_per_image.csv")
    assert per_image["mean_ap"].tolist() == [1.0] * 4 and per_image["n_pred"].tolist() == per_image["n_gt"].tolist()
    assert per_image["n_pred"].iloc[3] > 3 and per_image["pixel_iou"].tolist() == [1.0] * 4
    gt_dir = write_gt(tmp_path / "gt", cli_gt_masks())
    kept = [int((areas(B, kmax(B)) >= 30).sum()) for B in (cc_labels(m) for m in cli_gt_masks())]
    out = run_cli(tmp_path, monkeypatch, "big", ["--gt_dir", str(gt_dir), "--gt_min_area", "30"])
    assert pd.read_csv(out / "match_per_image.csv")["n_gt"].tolist() == kept + [sum(kept)]
    assert kept[1] < kmax(cc_labels(cli_gt_masks()[1]))


def test_cli_refuses_a_missing_or_misfit_mask_before_any_image(tmp_path, monkeypatch):
    run_cli(tmp_path, monkeypatch, "plain", [])                    # writes the images
    gt_dir = write_gt(tmp_path / "gt", cli_gt_masks())
    (gt_dir / "im1.png").unlink()
    with pytest.raises(SystemExit, match="im1"):
        run_cli(tmp_path, monkeypatch, "missing", ["--gt_dir", str(gt_dir)])
    assert not (tmp_path / "missing").exists()
    Image.fromarray(np.zeros((SIZE, SIZE + 1), np.uint8)).save(gt_dir / "im1.tif")
    with pytest.raises(SystemExit, match="im1.tif"):
        run_cli(tmp_path, monkeypatch, "misfit", ["--gt_dir", str(gt_dir)])
    assert not (tmp_path / "misfit").exists()
