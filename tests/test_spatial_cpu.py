"""CPU: Ripley's K of droplet centroids.  The host path utils/spatial_stats.py against the plain loops
of tests/spatial_ref.py, integer for integer; the hash against recorded values; the derived columns; what the statistics say
about a clustered, a regular and a random pattern; the CLI's CPU path."""
import numpy as np
import pytest

from tests import spatial_ref as ref
from utils import spatial_stats as ss

# u = hi * 2^32 + lo of (seed, s, k), computed once with Python integers from the definition (fmix32 is the MurmurHash3
# finaliser: fmix32(1) = 0x514e28b7 is the low half of the first entry)
RECORDED_U = {
    (0x0, 0, 0): 0x00000000514e28b7,
    (0x0, 0, 1): 0x30f4c30685f0b427,
    (0x0, 1, 0): 0xaa3e5b616f0b28e6,
    (0x1, 0, 0): 0x5716f995bb704eb1,
    (0x3039, 0, 0): 0xcf278ba91befd599,
    (0x3039, 3, 17): 0x6bfcf36adcb1d36f,
    (0x3039, 98, 1023): 0xd05f13b73531ecbd,
    (0xffffffff, 0, 0): 0xc733fe0f4f03351e,
    (0xffffffff, 998, 1048575): 0x9ad63d579162bbe2,
    (0x7, 1, 2): 0x50fd8edfa257dc80,
    (0x7, 2, 1): 0xb6b0957470bce881,
    (0x80000000, 5, 5): 0xf6030f37c51db905,
    (0x3ea, 0, 299): 0x7aa9d8c9d7338dea,
    (0x3eb, 38, 0): 0x79119f32f73a5f5c,
    (0x63, 99, 99): 0xe1c4fef482e405cd,
    (0xdeadbeef, 500, 65536): 0xdc0361b82839bf77,
}


def host_counts(pts, h, w, R, S, seed, window):
    py, px = [p[0] for p in pts], [p[1] for p in pts]
    return tuple(v.tolist() for v in ss.ripley_counts_numpy(py, px, h, w, R, S, seed, window))


def assert_equals_loops(pts, h, w, R, S, seed, window):
    got, want = host_counts(pts, h, w, R, S, seed, window), ref.ripley_counts(pts, h, w, R, S, seed, window)
    for name, g, v in zip(("n", "pairs", "pairs_all"), got, want):
        assert g == v, (name, R, S)
    return want


@pytest.mark.parametrize("name", sorted(ref.hand_fixtures()))
def test_hand_fixtures(name):
    pts, h, w, R, window, checks = ref.hand_fixtures()[name]
    n, pairs, pairs_all = assert_equals_loops(pts, h, w, R, 3, 5, window)
    if "c" in checks:
        assert ref.pair_radius(pts[0], pts[1]) == checks["c"]
    zeros = [] if window is None else [tuple(q) for q in np.argwhere(window == 0).tolist()]
    if "e" in checks:
        d2w = None if window is None or window.all() else ss.edt_sq(window)
        es = [ref.border_radius(p, h, w, R, zeros) for p in pts]
        assert es == checks["e"] == ss.border_radius([p[0] for p in pts], [p[1] for p in pts], h, w, R, d2w).tolist()
        assert n[0] == [sum(e >= r for e in es) for r in range(R + 1)]
    for r, want in checks.get("pairs_all", {}).items():
        assert pairs_all[0][r] == want, r
    assert all(row[r] <= allrow[r] for row, allrow in zip(pairs, pairs_all) for r in range(R + 1))
    if len(pts) == 0:
        assert all(v == 0 for q in (n, pairs, pairs_all) for row in q for v in row)


def test_window_cases_of_the_definition():
    f = ref.hand_fixtures()
    pts, h, w, R, ones, _ = f["all_ones_window"]
    assert host_counts(pts, h, w, R, 3, 9, ones) == host_counts(pts, h, w, R, 3, 9, None)       # D2 = INF: equal to NULL
    one = f["one_pixel_window"][4]
    area, sy, sx = np.array([1, 4, 2]), np.array([3, 12, 0]), np.array([4, 16, 0])
    py, px, info = ss.droplet_points(area, sy, sx, 7, 9, one)
    assert (py.tolist(), px.tolist(), info) == ([3, 3], [4, 4], {"N": 2, "n_dropped": 1, "A": 1})   # (0, 0) is outside W
    assert ref.points_of_table(area, sy, sx, 7, 9, one.tolist()) == ([(3, 4), (3, 4)], 1)
    for s in range(3):                                          # a one-pixel window: every simulated point lands on it
        y, x = ss.simulated_points(11, s, 5, 7, 9, one)
        assert y.tolist() == [3] * 5 and x.tolist() == [4] * 5
    n, pairs, pairs_all = ss.ripley_counts_numpy(py, px, 7, 9, 3, 2, 11, one)
    assert pairs_all.tolist() == [[2] * 4] * 3 and pairs.tolist() == [[2, 0, 0, 0]] * 3 and n.tolist() == [[2, 0, 0, 0]] * 3
    empty = np.zeros((7, 9), np.uint8)                          # A = 0: nothing is kept, every row is zero
    py, px, info = ss.droplet_points(area, sy, sx, 7, 9, empty)
    assert info == {"N": 0, "n_dropped": 3, "A": 0}
    assert all(not v.any() for v in ss.ripley_counts_numpy(py, px, 7, 9, 3, 2, 11, empty))


def test_centroids_round_half_up():
    area, sy, sx = np.array([2, 2, 3, 1]), np.array([1, 3, 4, 5]), np.array([9, 1, 4, 0])
    py, px, _ = ss.droplet_points(area, sy, sx, 20, 20)
    assert py.tolist() == [1, 2, 1, 5] and px.tolist() == [5, 1, 1, 0]        # 0.5 -> 1, 1.5 -> 2, 4/3 -> 1; 4.5 -> 5
    assert ref.points_of_table(area, sy, sx, 20, 20)[0] == list(zip(py.tolist(), px.tolist()))


@pytest.mark.parametrize("kind", ["null", "noisy", "holes"])
@pytest.mark.parametrize("hw", [(37, 53), (96, 130)])
def test_random_cases(hw, kind):
    h, w = hw
    area, sy, sx, window = ref.random_case(h, w, 70 if h > 40 else 33, kind, seed=h + len(kind))
    py, px, info = ss.droplet_points(area, sy, sx, h, w, window)
    pts, dropped = ref.points_of_table(area, sy, sx, h, w, None if window is None else window.tolist())
    assert list(zip(py.tolist(), px.tolist())) == pts and info["n_dropped"] == dropped and info["N"] == len(pts)
    assert info["A"] == len(ref.window_pixels(None if window is None else window.tolist(), h, w))
    assert dropped == 0 if kind == "null" else dropped > 0 or kind == "holes"
    for R in (1, 2, 5, 64):
        for S in (0, 1, 3):
            n, pairs, pairs_all = assert_equals_loops(pts, h, w, R, S, 40 + R, window)
            assert len(n) == 1 + S and pairs_all[0][R] > 0


def test_hash_recorded_values():
    assert len(RECORDED_U) == 16
    for (seed, s, k), u in RECORDED_U.items():
        assert ref.hash_u(seed, s, k) == u
        assert int(ss.hash_u(seed, s, np.array([k]))[0]) == u
    k = np.arange(300)
    assert ss.hash_u(1002, 7, k).tolist() == [ref.hash_u(1002, 7, int(q)) for q in k]
    for A in (1, 3, 12480, 2 ** 30 - 1):
        assert ss.draw_indices(1002, 7, 300, A).tolist() == [(ref.hash_u(1002, 7, int(q)) * A) >> 64 for q in k]


def test_selection_across_a_block_boundary_and_on_the_last_pixel():
    h, w = 6, 130
    win = np.zeros((h, w), np.uint8)
    win[0, 63] = win[0, 64] = win[2, 127] = win[2, 128] = win[h - 1, w - 1] = 1
    inside = ref.window_pixels(win.tolist(), h, w)
    assert inside[-1] == (h - 1, w - 1) and len(inside) == 5
    seen = set()
    for s in range(4):
        y, x = ss.simulated_points(3, s, 40, h, w, win)
        got = list(zip(y.tolist(), x.tolist()))
        assert got == ref.simulated(3, s, 40, inside)
        seen |= set(got)
    assert seen == set(inside)                                  # every pixel of W is drawn, the last one included
    y, x = ss.simulated_points(3, 0, 500, h, w, None)
    assert list(zip(y.tolist(), x.tolist())) == ref.simulated(3, 0, 500, ref.window_pixels(None, h, w))


def disc_count(r):
    """Lattice points within r of a lattice point, itself included."""
    return sum(1 for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r)


def test_ripley_columns():
    c = ss.ripley_columns([3, 2, 0], [0, 4, 0], [0, 4, 6], A=100, N=3)
    assert c["K"][1] == 100 * 4 / (2 * 2) and np.isnan(c["K"][2]) and c["K"][0] == 0.0            # n[r] = 0 -> NaN
    assert c["L"][1] == np.sqrt(100 / np.pi) and c["L_minus_r"][1] == c["L"][1] - 1 and np.isnan(c["L"][2])
    assert np.isnan(c["g"][0]) and c["g"][1] == (c["K"][1] - c["K"][0]) / np.pi and np.isnan(c["g"][2])
    assert c["K_raw"].tolist() == [0.0, 100 * 4 / 6, 100.0]
    for N in (0, 1):                                            # N < 2 -> NaN everywhere
        c = ss.ripley_columns([N, N], [0, 0], [0, 0], A=50, N=N)
        assert all(np.isnan(c[q]).all() for q in ("K", "L", "L_minus_r", "g", "K_raw"))
    # one point on every pixel of a 31 x 29 window: an eligible point sees the whole disc, so K (N - 1) / A is the lattice disc
    # count without the point itself, at every r with an eligible point
    h, w, R = 31, 29, 9
    yy, xx = np.mgrid[0:h, 0:w]
    n, pairs, pairs_all = ss.ripley_counts_numpy(yy.ravel(), xx.ravel(), h, w, R, 0, 0)
    c = ss.ripley_columns(n[0], pairs[0], pairs_all[0], h * w, h * w)
    for r in range(R + 1):
        assert n[0][r] == (h - 2 * r) * (w - 2 * r) and pairs[0][r] == n[0][r] * (disc_count(r) - 1)
        assert abs(c["K"][r] * (h * w - 1) / (h * w) - (disc_count(r) - 1)) < 1e-9
    assert disc_count(1) - 1 == 4                               # K(1) counts the 4 neighbours: small r is lattice-jagged


def test_envelope_rules():
    lo, hi, mean = ss.envelope(np.array([[0.0, 1.0, np.nan], [0.0, 3.0, np.nan], [0.0, np.nan, np.nan]]))
    assert lo.tolist()[:2] == [0.0, 1.0] and hi.tolist()[:2] == [0.0, 3.0] and mean.tolist()[:2] == [0.0, 2.0]
    assert np.isnan(lo[2]) and np.isnan(hi[2]) and np.isnan(mean[2])
    assert all(np.isnan(v).all() for v in ss.envelope(np.zeros((0, 4))))


H, W = 300, 401


def analysed(py, px, R, S, seed=12345):
    n, pairs, pairs_all = ss.ripley_counts_numpy(py, px, H, W, R, S, seed)
    return ss.analyse(n, pairs, pairs_all, H * W, len(py))


def test_a_clustered_pattern_reads_clustered():
    rng = np.random.default_rng(12345)
    parents = np.stack([rng.integers(6, H - 6, 40), rng.integers(6, W - 6, 40)], axis=1)
    pts = (parents[:, None, :] + rng.integers(-6, 7, (40, 10, 2))).reshape(-1, 2)
    res = analysed(pts[:, 0], pts[:, 1], 32, 99)
    assert res["csr_p"] == 0.01 and res["pattern"] == "clustered"
    for r in (4, 8, 16):
        assert res["L_minus_r"][r] > res["env_hi"][r] and res["outside"][r] == 1


def test_a_lattice_reads_regular():
    yy, xx = np.mgrid[7:H:15, 7:W:15]
    assert yy.size == 540
    res = analysed(yy.ravel(), xx.ravel(), 32, 99)
    assert res["csr_p"] == 0.01 and res["pattern"] == "regular"
    assert all(res["L_minus_r"][r] == -r for r in range(1, 15)) and res["L_minus_r"][15] > -15
    assert all(res["outside"][r] == -1 for r in range(6, 15))


RANDOM_FIXTURE_P = 0.925       # csr_p of 300 points drawn by the definition's own generator from seed 1002, on the numpy path


def test_a_random_pattern_reads_random():
    py, px = ss.simulated_points(1002, 0, 300, H, W)
    res = analysed(py, px, 16, 39)
    assert res["csr_p"] == RANDOM_FIXTURE_P >= 0.2 and res["pattern"] == "random"
    assert analysed(py, px, 16, 0)["pattern"] == "" and np.isnan(analysed(py, px, 16, 0)["csr_p"])


def test_rows_of_the_two_tables():
    py, px = ss.simulated_points(5, 0, 60, 64, 80)
    rec = ss.spatial_record(np.ones(60, np.int64), py, px, 64, 80, 5, 3, 1)
    res = ss.analyse(rec["n"], rec["pairs"], rec["pairs_all"], rec["A"], rec["N"])
    rows = ss.table_rows("a.png", (rec["n"], rec["pairs"], rec["pairs_all"]), res, 2.0)
    assert [r["r_px"] for r in rows] == [1, 2, 3, 4, 5] and rows[1]["r_micron"] == 1.0
    assert tuple(rows[0]) == ss.table_columns(2.0) and tuple(ss.table_rows("a.png", (rec["n"], rec["pairs"], rec["pairs_all"]), res)[0]) == ss.TABLE_COLUMNS
    row = ss.summary_row("a.png", rec, res)
    assert tuple(row) == ss.IMAGE_COLUMNS and row["n_points"] == 60 and row["window_px"] == 64 * 80
    assert row["droplets_per_10k_px"] == 1e4 * 60 / (64 * 80)
    for bad in (0, 257, 1.5, True):
        with pytest.raises(ValueError):
            ss.check_radius(bad)
    assert ss.check_radius(256) == 256 and ss.check_sims(0) == 0 and ss.check_sims(999) == 999
    with pytest.raises(ValueError):
        ss.check_sims(1000)


def test_cli_cpu_path_writes_both_files_and_nothing_else_changes(tmp_path, monkeypatch):
    import pandas as pd
    from PIL import Image
    from tests.test_split_cpu import files, run_cli
    plain = run_cli(tmp_path, monkeypatch, "plain", ["--px_per_micron", "2.0"])
    on = run_cli(tmp_path, monkeypatch, "on", ["--px_per_micron", "2.0", "--spatial_stats", "6", "--spatial_sims", "3", "--spatial_seed", "4"])
    assert sorted(set(files(on)) - set(files(plain))) == ["spatial_per_image.csv", "spatial_stats.csv"]
    assert not any("spatial" in f for f in files(plain))
    for f in files(plain):                                      # the flag adds two files and changes no byte of the others
        assert (plain / f).read_bytes() == (on / f).read_bytes(), f
    per = pd.read_csv(on / "spatial_per_image.csv")
    table = pd.read_csv(on / "spatial_stats.csv")
    assert tuple(per.columns) == ss.IMAGE_COLUMNS and tuple(table.columns) == ss.table_columns(2.0)
    assert len(per) == 3 and len(table) == 3 * 6 and table["r_px"].tolist() == [1, 2, 3, 4, 5, 6] * 3
    summary = pd.read_csv(on / "summary_per_image.csv")
    assert per["n_points"].tolist() == summary["droplet_count"].tolist()
    # a window that holds nothing: every droplet is dropped; and a missing window ends the run before anything is written
    import quantify_droplets_batch as q
    wdir = tmp_path / "windows"
    wdir.mkdir()
    for i in range(3):
        Image.fromarray(np.zeros(Image.open(tmp_path / "imgs" / f"im{i}.png").size[::-1], np.uint8)).save(wdir / f"im{i}.png")
    win = run_cli(tmp_path, monkeypatch, "win", ["--spatial_stats", "--spatial_sims", "0", "--spatial_window_dir", str(wdir)])
    per = pd.read_csv(win / "spatial_per_image.csv")
    assert per["n_points"].tolist() == [0, 0, 0] and per["n_dropped"].tolist() == summary["droplet_count"].tolist()
    assert len(pd.read_csv(win / "spatial_stats.csv")) == 3 * 64
    (wdir / "im1.png").unlink()
    with pytest.raises(SystemExit, match="--spatial_window_dir"):
        run_cli(tmp_path, monkeypatch, "missing", ["--spatial_stats", "--spatial_window_dir", str(wdir)])
    assert not (tmp_path / "missing").exists()
    for bad in (["--spatial_stats", "0"], ["--spatial_stats", "257"]):
        with pytest.raises(SystemExit):
            q.build_parser().parse_args(["--img_dir", "x", *bad])
    with pytest.raises(SystemExit, match="spatial_sims"):
        run_cli(tmp_path, monkeypatch, "bad", ["--spatial_stats", "--spatial_sims", "1000"])
