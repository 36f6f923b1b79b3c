"""CPU: the confidence rule (utils/droplet_confidence.py) against its independent restatement
(tests/confidence_ref.py), the facts of the entropy table and of the quantisation, the envelope of utils.tta.mean_env_numpy, the
column formulas on a case computed by hand, and quantify_droplets_batch.py --confidence on the script's CPU path."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from tests.confidence_ref import IMAGE_NAMES, NAMES, confidence_ref, quant_ref
from utils import droplet_confidence as dc
from utils import tta

THRESH, BAND = 0.3, 0.1


def label_map(oh, ow, seed, n_labels=6):
    """Blocks of 3 x 5 pixels with random labels 0..n_labels: touching labels, runs of every length, background."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, n_labels + 1, ((oh + 2) // 3, (ow + 4) // 5))
    small[rng.random(small.shape) < 0.4] = 0
    return np.repeat(np.repeat(small, 3, 0), 5, 1)[:oh, :ow].astype(np.int32)


def planes(ph, pw, seed, thresh=THRESH, band=BAND):
    """(probs, lo, hi) fp32 [ph, pw]: random probabilities with the special values sprinkled in (exactly the threshold, the
    threshold +- the band, 0, 1, NaN, below 0, above 1); an envelope around them that leaves [0, 1] in places."""
    rng = np.random.default_rng(seed)
    p = rng.random((ph, pw), dtype=np.float32)
    t, b = np.float32(thresh), np.float32(band)
    special = np.array([t, t + b, t - b, 0.0, 1.0, np.nan, -0.5, 1.5, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))], np.float32)
    at = rng.random((ph, pw)) < 0.3
    p[at] = special[rng.integers(0, len(special), int(at.sum()))]
    base = np.where(np.isnan(p), np.float32(0.4), p)
    lo = (base - rng.random((ph, pw), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
    hi = (base + rng.random((ph, pw), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
    same = rng.random((ph, pw)) < 0.2
    hi[same] = lo[same]
    return p, lo, hi


@functools.lru_cache(maxsize=None)
def fixture(oh, ow, ph, pw):
    lab = label_map(oh, ow, seed=oh * 1000 + ow)
    p, lo, hi = planes(ph, pw, seed=ph * 1000 + pw + 1)
    if (oh, ow) == (ph, pw) and ow >= 64:                       # a full chunk and a row-long run of p = 1.0: q^2 partials past 2^31
        lab[0, :], lab[oh - 1, :64] = 2, 3
        p[0, :] = p[oh - 1, :64] = 1.0
    if oh > 4 and ow > 6:
        lab[1, 1], lab[2, 3], lab[3, 5] = 9, -4, 2 ** 31 - 1    # above max_out and negative: skipped in the rows
    for a in (lab, p, lo, hi):
        a.setflags(write=False)
    return lab, p, lo, hi


# (oh, ow, ph, pw): the identity geometry at the wave-chunk edges, and two resizes
GEOMETRIES = [(1, 1, 1, 1), (1, 64, 1, 64), (37, 53, 37, 53), (64, 64, 64, 64), (96, 130, 96, 130), (5, 63, 5, 63), (5, 65, 5, 65),
              (3, 129, 3, 129), (37, 53, 16, 16), (96, 130, 64, 64)]
MAX_OUT = 6


def assert_equals_ref(rec, ref):
    rows, image, hmap, smap = ref
    for name in NAMES:
        assert rec[name].dtype == np.int64 and [int(v) for v in rec[name]] == rows[name], name
    assert [int(v) for v in rec["image"]] == [image[q] for q in IMAGE_NAMES]
    assert np.array_equal(rec["entropy_u8"], hmap)
    if rec["envelope"]:
        assert np.array_equal(rec["spread_u8"], smap)
    else:
        assert rec["spread_u8"] is None


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("envelope", [False, True])
def test_host_path_equals_restatement(geometry, envelope):
    lab, p, lo, hi = fixture(*geometry)
    env = dict(lo=lo, hi=hi) if envelope else {}
    rec = dc.confidence_numpy(lab, p, THRESH, BAND, max_out=MAX_OUT, maps=True, **env)
    assert_equals_ref(rec, confidence_ref(lab, p, THRESH, BAND, max_out=MAX_OUT, **env))
    assert tuple(dc.CONF_QUANTITIES) == NAMES and tuple(dc.IMAGE_QUANTITIES) == IMAGE_NAMES
    if not envelope:
        for name in dc.ENVELOPE_QUANTITIES:
            assert np.all(rec[name] == (-1 if name.startswith("max_") else 0))


@pytest.mark.parametrize("band", [0.0, 0.5])
def test_band_limits_and_default_capacity(band):
    lab, p, lo, hi = fixture(37, 53, 16, 16)
    small = np.where((lab > 0) & (lab <= 9), lab, 0)
    rec = dc.confidence_numpy(small, p, 0.5, band, lo, hi, maps=True)
    assert len(rec["n"]) == 9                                                   # without max_out: the largest label
    assert_equals_ref(rec, confidence_ref(small, p, 0.5, band, lo, hi))
    if band == 0.0:
        assert rec["image"][4] == int((dc.quant(p)[dc.sample_index(37, 16)[:, None], dc.sample_index(53, 16)[None, :]] == 32768).sum())
    for bad in (-0.01, 0.51, float("nan"), True, "0.1", None):
        with pytest.raises(ValueError):
            dc.check_band(bad)
    with pytest.raises(ValueError):
        dc.confidence_numpy(small, p, 0.5, 0.1, lo=lo)


def test_entropy_table_facts():
    t = dc.entropy_table()
    assert t.dtype == np.uint16 and t.shape == (65536,)
    assert t[0] == t[65535] == 0 and t[32767] == t[32768] == 65535
    assert np.array_equal(t, t[::-1])
    assert np.all(np.diff(t[:32768].astype(np.int64)) >= 0)
    # no entry near a rounding tie: another libm cannot move it
    p = np.arange(1, 65535, dtype=np.float64) / 65535
    x = 65535 * -(p * np.log2(p) + (1 - p) * np.log2(1 - p))
    assert np.abs(x - np.floor(x) - 0.5).min() > 5e-7
    for q in (1, 2, 100, 6553, 32767, 50000, 65534):
        from tests.confidence_ref import entropy16_ref
        assert int(t[q]) == entropy16_ref(q)


def test_quantisation_edges_and_the_fp32_product():
    q = dc.quant(np.array([0.0, 1.0, np.nan, -1.0, -0.0, 2.0, np.inf, -np.inf, 0.5, 1e-6], np.float32))
    assert q.dtype == np.int64 and q.tolist() == [0, 65535, 0, 0, 0, 65535, 65535, 0, 32768, 0]
    assert dc.quant(np.float32(0.3)) == quant_ref(np.float32(0.3)) and dc.quant(0.3) == dc.quant(np.float32(0.3))
    p = np.random.default_rng(5).random(1 << 20, dtype=np.float32)
    q32 = dc.quant(p)
    q64 = np.rint(p.astype(np.float64) * 65535.0).astype(np.int64)
    differ = np.flatnonzero(q32 != q64)
    print(f"[quant] {differ.size} of 2^20 random fp32 inputs quantise differently under a float64 product")
    assert 100 < differ.size < 10000 and np.all(np.abs(q32[differ] - q64[differ]) == 1)
    for i in differ[:300]:                                  # the rule is the fp32 product: the scalar restatement agrees there
        assert int(q32[i]) == quant_ref(p[i])
    assert np.all(np.diff(dc.quant(np.sort(p))) >= 0)       # monotone: spread = quant(hi) - quant(lo) >= 0


@pytest.mark.parametrize("N", [1, 2, 4, 8])
def test_mean_env_numpy(N):
    p = np.random.default_rng(N).random((3 * N, 32, 32), dtype=np.float32)
    mean, lo, hi = tta.mean_env_numpy(p, N)
    assert np.array_equal(mean.view(np.uint32), tta.mean_numpy(p, N).view(np.uint32))
    back = np.stack([np.stack([tta.variant_inverse(p[b * N + i], v) for i, v in enumerate(tta.variants(N))]) for b in range(3)])
    assert np.array_equal(lo, back.min(1)) and np.array_equal(hi, back.max(1)) and np.all(lo <= hi)
    assert lo.dtype == hi.dtype == np.float32 and lo.flags.c_contiguous and hi.flags.c_contiguous
    if N == 1:
        assert np.array_equal(lo, p) and np.array_equal(hi, p)


def test_the_mean_of_equal_values_may_leave_the_envelope():
    """Not an invariant: eight sequential fp32 adds of one value, divided by 8, miss the value for many values."""
    v = np.random.default_rng(0).random(4096, dtype=np.float32)
    acc = v.copy()
    for _ in range(7):
        acc = acc + v
    assert 0.1 < float(((acc / np.float32(8)) != v).mean()) < 0.9


def test_columns_on_a_case_computed_by_hand():
    lab = np.array([[1, 1, 0, 2, 2], [3, 3, 3, 0, 0]], np.int32)
    p = np.array([[1.0, 1.0, 0.5, 0.0, 1.0], [0.5, 0.5, 1.0, 0.0, 0.25]], np.float32)
    lo = np.array([[1.0, 0.5, 0.5, 0.0, 0.0], [0.5, 0.25, 1.0, 0.0, 0.25]], np.float32)
    hi = np.array([[1.0, 1.0, 0.5, 0.0, 1.0], [0.5, 1.0, 1.0, 0.0, 0.25]], np.float32)
    rec = dc.confidence_numpy(lab, p, 0.5, 0.1, lo, hi)
    Q, H = 65535, 32768                                     # q(0.5) = rint(32767.5) = 32768 (half to even), H16 = 65535 there
    assert rec["n"].tolist() == [2, 2, 3] and rec["Sq"].tolist() == [2 * Q, Q, 2 * H + Q]
    assert rec["Sqq"].tolist() == [2 * Q * Q, Q * Q, 2 * H * H + Q * Q]
    assert rec["min_q"].tolist() == [Q, 0, H] and rec["max_q"].tolist() == [Q, Q, Q]
    assert rec["n_band"].tolist() == [0, 0, 2] and rec["Sh"].tolist() == [0, 0, 2 * Q]
    assert rec["Sspread"].tolist() == [Q - H, Q, Q - 16384] and rec["max_spread"].tolist() == [Q - H, Q, Q - 16384]
    assert rec["n_unstable"].tolist() == [1, 1, 1]          # lo = 0.5 is not above the threshold 0.5, hi = 1.0 is
    q25 = 16384                                             # rint(16383.75)
    h25 = int(dc.entropy_table()[q25])
    assert rec["image"].tolist() == [10, 7, 3 * Q + h25, 2 * Q, 3, 2, 3, (Q - H) + Q + (Q - q25)]
    c = dc.confidence_columns(rec)
    assert list(c) == ["prob_mean", "prob_std", "prob_min", "prob_max", "entropy_mean", "uncertain_frac", "tta_spread_mean",
                       "tta_spread_max", "unstable_frac"]
    assert c["prob_mean"].tolist() == [1.0, 0.5, (2 * H + Q) / (3 * Q)] and c["prob_std"][:2].tolist() == [0.0, 0.5]
    m3 = (2 * H + Q) / 3
    assert c["prob_std"][2] == np.sqrt(max((2 * H * H + Q * Q) / 3 - m3 * m3, 0.0)) / Q
    assert c["prob_min"].tolist() == [1.0, 0.0, H / Q] and c["prob_max"].tolist() == [1.0, 1.0, 1.0]
    assert c["entropy_mean"].tolist() == [0.0, 0.0, 2 / 3] and c["uncertain_frac"].tolist() == [0.0, 0.0, 2 / 3]
    assert c["tta_spread_mean"].tolist() == [(Q - H) / (2 * Q), 0.5, (Q - q25) / (3 * Q)]
    assert c["tta_spread_max"].tolist() == [(Q - H) / Q, 1.0, (Q - q25) / Q] and c["unstable_frac"].tolist() == [0.5, 0.5, 1 / 3]
    row = dc.image_columns(rec)
    assert list(row) == list(dc.IMAGE_COLUMNS)
    assert row["entropy_mean"] == (3 * Q + h25) / (10 * Q) and row["entropy_mean_bg"] == (Q + h25) / (3 * Q)
    assert (row["uncertain_px"], row["uncertain_bg_px"], row["unstable_px"], row["droplets"]) == (3, 1, 3, 3)
    assert row["tta_spread_mean"] == ((Q - H) + Q + (Q - q25)) / (10 * Q) and row["min_droplet_prob_mean"] == 0.5
    plain = dc.confidence_numpy(lab, p, 0.5, 0.1)
    assert list(dc.confidence_columns(plain)) == list(c)[:6]
    r = dc.image_columns(plain)
    assert np.isnan(r["unstable_px"]) and np.isnan(r["tta_spread_mean"]) and r["uncertain_px"] == 3
    empty = dc.confidence_numpy(np.zeros((2, 5), np.int32), p, 0.5, 0.1)
    assert len(empty["n"]) == 0 and np.isnan(dc.image_columns(empty)["min_droplet_prob_mean"])


def test_droplet_options_carry_the_band():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.droplets import DropletOptions
    assert DropletOptions().confidence is None and not DropletOptions().confidence_maps
    o = DropletOptions(confidence=0.1, confidence_maps=True, labels=True)     # the confidence route has a label map
    assert o.confidence == 0.1 and o.label_map and not DropletOptions().label_map
    for bad in (dict(confidence=0.6), dict(confidence=-0.1), dict(confidence_maps=True)):
        with pytest.raises(_lib.UnetdcError):
            DropletOptions(**bad)


# ---- the script ------------------------------------------------------------------------------------------------------------------

def disc_images(sizes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        img = (rng.random((h, w, 3)) * 60).astype(np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        for _ in range(7):
            cy, cx, r = rng.integers(6, h - 6), rng.integers(6, w - 6), rng.integers(3, 9)
            img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = (230, 200, 170)
        out.append(img)
    return out


def run_script(tmp_path, monkeypatch, tag, extra, device="cpu", sizes=((96, 96), (80, 112), (64, 64)), img_size=64):
    """quantify_droplets_batch.main on synthetic disc images; the network is tests.test_tta_cpu.fake_model, which is exact and
    gives the same bits in any batch on either device."""
    import quantify_droplets_batch as q
    from tests.test_tta_cpu import fake_model
    monkeypatch.setattr(q, "DEVICE", device)
    monkeypatch.setattr(q, "IMG_SIZE", img_size)
    monkeypatch.setattr(q, "load_model", lambda ckpt, dtype="f32": fake_model)
    img_dir = tmp_path / "imgs"
    if not img_dir.exists():
        img_dir.mkdir()
        for i, img in enumerate(disc_images(sizes)):
            Image.fromarray(img).save(img_dir / f"im{i}.png")
    return q.main(["--img_dir", str(img_dir), "--out_dir", str(tmp_path / tag), "--batch", "2", "--skip_excel", "--skip_histogram",
                   "--background_radius", "15", "--prob_thresh", "0.3", "--min_area", "2", *extra])


def files(d):
    return sorted(str(p.relative_to(d)) for p in d.rglob("*") if p.is_file())


BASE_COLUMNS = ["filename", "label", "area", "equivalent_diameter", "centroid-0", "centroid-1"]
CONF_COLUMNS = ["prob_mean", "prob_std", "prob_min", "prob_max", "entropy_mean", "uncertain_frac"]
TTA_COLUMNS = ["tta_spread_mean", "tta_spread_max", "unstable_frac"]


def test_script_cpu_path(tmp_path, monkeypatch):
    from utils import droplet_confidence
    with monkeypatch.context() as mp:                        # without the flag the stage's code is never reached
        mp.setattr(droplet_confidence, "confidence_numpy", None)
        mp.setattr(droplet_confidence, "confidence_columns", None)
        plain = run_script(tmp_path, mp, "plain", [])
    assert files(plain) == sorted(["all_droplets.csv", "droplet_size_stats.csv", "summary_per_image.csv"] +
                                  [f"im{i}_droplets.csv" for i in range(3)] + [f"predicted_masks/im{i}_pred.png" for i in range(3)])
    assert list(pd.read_csv(plain / "all_droplets.csv").columns) == BASE_COLUMNS
    conf = run_script(tmp_path, monkeypatch, "conf", ["--confidence"])
    assert sorted(set(files(conf)) - set(files(plain))) == ["confidence_per_image.csv"]
    for f in files(plain):                                   # the stage reads; nothing the flow computed before moves
        if not f.endswith("droplets.csv"):
            assert (plain / f).read_bytes() == (conf / f).read_bytes(), f
    a, b = pd.read_csv(plain / "all_droplets.csv"), pd.read_csv(conf / "all_droplets.csv")
    assert list(b.columns) == BASE_COLUMNS + CONF_COLUMNS and len(b) > 6 and b[BASE_COLUMNS].equals(a)
    assert b["prob_mean"].between(0, 1).all() and (b["prob_min"] <= b["prob_mean"]).all() and (b["prob_mean"] <= b["prob_max"]).all()
    per = pd.read_csv(conf / "confidence_per_image.csv")
    assert list(per.columns) == ["filename"] + list(dc.IMAGE_COLUMNS) and per["filename"].tolist() == [f"im{i}.png" for i in range(3)]
    assert per["droplets"].tolist() == [int((b["filename"] == f"im{i}.png").sum()) for i in range(3)]
    assert per["unstable_px"].isna().all() and (per["uncertain_bg_px"] <= per["uncertain_px"]).all()
    # with --tta the envelope columns and the maps; the band enters uncertain_frac alone
    both = run_script(tmp_path, monkeypatch, "both", ["--confidence", "0.2", "--tta", "4", "--confidence_maps"])
    c = pd.read_csv(both / "all_droplets.csv")
    assert list(c.columns) == BASE_COLUMNS + CONF_COLUMNS + TTA_COLUMNS and (c["tta_spread_max"] >= c["tta_spread_mean"]).all()
    assert c["tta_spread_max"].max() > 0
    per = pd.read_csv(both / "confidence_per_image.csv")
    assert per["unstable_px"].notna().all() and per["tta_spread_mean"].gt(0).all()
    for i, (h, w) in enumerate(((96, 96), (80, 112), (64, 64))):
        for kind in ("entropy", "spread"):
            m = np.array(Image.open(both / f"im{i}_{kind}.png"))
            assert m.shape == (h, w) and m.dtype == np.uint8
    tiled = run_script(tmp_path, monkeypatch, "tiled", ["--confidence", "--tta", "2", "--tile", "64", "--tile_overlap", "16"])
    assert list(pd.read_csv(tiled / "all_droplets.csv").columns) == BASE_COLUMNS + CONF_COLUMNS + TTA_COLUMNS
    for bad in (["--confidence", "0.7"], ["--confidence_maps"]):
        with pytest.raises(SystemExit):
            run_script(tmp_path, monkeypatch, "bad", bad)


def test_script_combinations_on_the_cpu_path(tmp_path, monkeypatch):
    """The stage reads only the final label map: with the split, shape, neighbours, cleaning and annotations the record is that of
    confidence_numpy on the labels the flow wrote."""
    from utils.droplet_split import labels_u16  # noqa: F401  (the label images of --split_touching are read back below)
    out = run_script(tmp_path, monkeypatch, "combo", ["--confidence", "--split_touching", "--droplet_shape", "--neighbors", "3",
                                                      "--fill_holes"])
    t = pd.read_csv(out / "all_droplets.csv")
    assert set(CONF_COLUMNS) <= set(t.columns) and "perimeter" in t.columns and "nn_label" in t.columns
    lab = np.array(Image.open(out / "predicted_masks" / "im2_labels.png")).astype(np.int32)
    rows = t[t["filename"] == "im2.png"]
    assert len(rows) == lab.max() and np.array_equal(np.bincount(lab.ravel())[1:], rows["area"].to_numpy())
