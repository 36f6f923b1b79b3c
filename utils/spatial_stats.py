"""Ripley's K / L of the droplet centroids with a Monte Carlo envelope of complete spatial randomness: the whole definition
of DESIGN.md section 26 on the host, in integers up to the counts and in float64 behind them.  It is the CPU path of
``quantify_droplets_batch.py --spatial_stats`` and the yardstick of the device path (csrc/spatial.hip,
unet_dc_segmentation_amd/spatial.py: bit-exact, tests/test_gpu_spatial.py); tests/spatial_ref.py restates it as plain loops.

    droplet_points        droplet table -> centroid pixels inside the window, in table order
    ripley_counts_numpy   points -> n[r], pairs[r], pairs_all[r] of the observed pattern (row 0) and of S simulated ones
    ripley_columns        one row of counts -> K, L, L - r, g, K_raw (float64; the ONLY place that forms them)
    envelope, analyse     the simulations' L - r -> env_lo / env_hi / env_mean, the global test, the pattern
    summary_row, table_rows   the rows of spatial_per_image.csv and spatial_stats.csv
"""
from __future__ import annotations

import numpy as np

from utils.droplet_split import edt_sq

MAX_RADIUS = 256
MAX_SIMS = 999
MAX_POINTS = 1 << 20
DEFAULT_RADIUS = 64         # a convention, not a measured number
GOLDEN = 0x9E3779B9
ALPHA = 0.05                # csr_p at or below it names the pattern clustered or regular
_M32 = np.uint64(0xFFFFFFFF)

TABLE_COLUMNS = ("filename", "r_px", "n_eligible", "pairs", "K", "L", "L_minus_r", "g", "K_raw", "env_lo", "env_hi", "env_mean",
                 "outside")
IMAGE_COLUMNS = ("filename", "n_points", "n_dropped", "window_px", "droplets_per_10k_px", "csr_p", "r_max_dev", "max_dev",
                 "pattern")


def check_radius(R):
    """-> R as int; ValueError for what unetdc_ripley_counts refuses (an integer 1..256)."""
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= int(R) <= MAX_RADIUS:
        raise ValueError(f"the largest radius must be an integer in 1..{MAX_RADIUS} pixels, not {R!r}")
    return int(R)


def check_sims(S):
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 0 <= int(S) <= MAX_SIMS:
        raise ValueError(f"the number of simulations must be an integer in 0..{MAX_SIMS}, not {S!r}")
    return int(S)


def fmix32(h):
    """The 32-bit finaliser of csrc/hash32.h on uint64 arrays that hold 32-bit values."""
    h = np.asarray(h, np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def hash_halves(seed, s, k):
    """(hi, lo) of the 64-bit draw u = hi * 2^32 + lo of point k (an array) of simulation s."""
    rowkey = fmix32(fmix32(np.uint64(int(seed) & 0xFFFFFFFF)) ^ np.uint64((int(s) * GOLDEN) & 0xFFFFFFFF))
    k2 = np.asarray(k, np.uint64) * np.uint64(2)
    return fmix32(rowkey ^ k2), fmix32(rowkey ^ (k2 + np.uint64(1)))


def hash_u(seed, s, k):
    hi, lo = hash_halves(seed, s, k)
    return (hi << np.uint64(32)) | lo


def draw_indices(seed, s, n, A):
    """t[k] = (u[k] * A) div 2^64 for k = 0..n-1, int64; A < 2^30, so both partial products stay below 2^62."""
    hi, lo = hash_halves(seed, s, np.arange(n, dtype=np.uint64))
    a = np.uint64(A)
    return ((hi * a + ((lo * a) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def _isqrt(v):
    """floor(sqrt(v)) of non-negative int64 below 2^52: the float proposes, integer comparisons fix it."""
    v = np.asarray(v, np.int64)
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    return r


def _window(window, h, w):
    if window is None:
        return None
    win = np.asarray(window)
    if win.shape != (h, w):
        raise ValueError(f"the window is {win.shape}, the image {(h, w)}")
    return win != 0


def window_area(window, h, w):
    win = _window(window, h, w)
    return h * w if win is None else int(win.sum())


def droplet_points(area, sum_y, sum_x, h, w, window=None):
    """Droplet table -> (py, px int64 [N] in table order, {"N", "n_dropped", "A"}): the centroid rounded half up, dropped
    where the window (nonzero = inside; None: every pixel) does not hold it."""
    a = np.maximum(np.asarray(area, np.int64), 1)
    y = (2 * np.asarray(sum_y, np.int64) + a) // (2 * a)
    x = (2 * np.asarray(sum_x, np.int64) + a) // (2 * a)
    win = _window(window, h, w)
    keep = (np.asarray(sum_y, np.int64) >= 0) & (y < h) & (np.asarray(sum_x, np.int64) >= 0) & (x < w)
    if win is not None:
        keep[keep] = win[y[keep], x[keep]]
    return y[keep], x[keep], {"N": int(keep.sum()), "n_dropped": int((~keep).sum()), "A": window_area(window, h, w)}


def border_radius(py, px, h, w, rmax, d2w=None):
    """e(p): the largest r in 0..rmax with r^2 < b2(p), b2 = min(D2_W(p), m^2), m the distance to the outside of the image."""
    py, px = np.asarray(py, np.int64), np.asarray(px, np.int64)
    m = np.minimum(np.minimum(py + 1, px + 1), np.minimum(h - py, w - px))
    b2 = m * m
    if d2w is not None:
        b2 = np.minimum(b2, d2w[py, px].astype(np.int64))
    return np.minimum(_isqrt(np.maximum(b2 - 1, 0)), rmax)      # b2 = 0: a given point outside the window, no margin


def _set_counts(y, x, e, R):
    """(n, pairs, pairs_all) int64 [R + 1] of one point set."""
    N = len(y)
    H = np.zeros((R + 1) * (R + 1), np.int64)              # [e][c]
    step = max(1, (1 << 22) // max(N, 1))
    for i0 in range(0, N, step):
        i1 = min(N, i0 + step)
        d2 = (y[i0:i1, None] - y[None, :]) ** 2 + (x[i0:i1, None] - x[None, :]) ** 2
        near = d2 <= R * R
        near[np.arange(i1 - i0), np.arange(i0, i1)] = False
        ii, jj = np.nonzero(near)
        v = d2[ii, jj]
        r = _isqrt(v)
        c = r + (r * r < v)
        H += np.bincount(e[i0 + ii] * (R + 1) + c, minlength=H.size)
    C = np.cumsum(H.reshape(R + 1, R + 1), axis=1)          # [e][r]: pairs of a point of border radius e within r
    suffix = np.cumsum(C[::-1], axis=0)[::-1]               # summed over e' >= e
    n = np.cumsum(np.bincount(e, minlength=R + 1)[::-1])[::-1]
    return n.astype(np.int64), np.diagonal(suffix).copy(), C.sum(axis=0)


def simulated_points(seed, s, n, h, w, window=None, inside=None):
    """The n points of simulation s: the t-th pixel of the window in raster order, t = draw_indices.  inside: the raster
    indices of the window's pixels when the caller has them."""
    if window is None:
        return np.divmod(draw_indices(seed, s, n, h * w), w)
    inside = np.flatnonzero(_window(window, h, w)) if inside is None else inside
    return np.divmod(inside[draw_indices(seed, s, n, len(inside))], w)


def ripley_counts_numpy(py, px, h, w, rmax, n_sim, seed, window=None):
    """Points (inside the image and the window) -> n, pairs, pairs_all: int64 [(1 + S), R + 1]; row 0 is the observed
    pattern, row s + 1 simulation s (zero rows without a point or without a window pixel)."""
    R, S = check_radius(rmax), check_sims(n_sim)
    py, px = np.asarray(py, np.int64), np.asarray(px, np.int64)
    N = len(py)
    win = _window(window, h, w)
    d2w = None if win is None or win.all() else edt_sq(win)
    inside = None if win is None else np.flatnonzero(win)
    A = h * w if win is None else len(inside)
    out = np.zeros((3, 1 + S, R + 1), np.int64)
    for s in range(-1, S if N and A else 0):
        y, x = (py, px) if s < 0 else simulated_points(seed, s, N, h, w, win, inside)
        out[:, s + 1] = _set_counts(y, x, border_radius(y, x, h, w, R, d2w), R)
    return out[0], out[1], out[2]


def ripley_columns(n, pairs, pairs_all, A, N):
    """One row of counts ([R + 1] each) -> {"K", "L", "L_minus_r", "g", "K_raw"}, float64 [R + 1], NaN where undefined."""
    n, pairs, pairs_all = (np.asarray(v, np.float64) for v in (n, pairs, pairs_all))
    R = len(n) - 1
    r = np.arange(R + 1, dtype=np.float64)
    K = np.full(R + 1, np.nan)
    K_raw = np.full(R + 1, np.nan)
    if N >= 2:
        ok = n > 0
        K[ok] = float(A) * pairs[ok] / (float(N - 1) * n[ok])
        K_raw = float(A) * pairs_all / (float(N - 1) * float(N))
    L = np.sqrt(K / np.pi)
    g = np.full(R + 1, np.nan)
    g[1:] = (K[1:] - K[:-1]) / (np.pi * (2.0 * r[1:] - 1.0))
    return {"K": K, "L": L, "L_minus_r": L - r, "g": g, "K_raw": K_raw}


def envelope(rows):
    """rows: float64 [S, R + 1] of the simulations' L - r -> (env_lo, env_hi, env_mean) over the simulations whose value is
    defined at that r; NaN where none is (and everywhere with S = 0)."""
    rows = np.atleast_2d(np.asarray(rows, np.float64))
    ok = ~np.isnan(rows)
    cnt = ok.sum(axis=0)
    some = cnt > 0
    lo = np.where(some, np.where(ok, rows, np.inf).min(axis=0, initial=np.inf), np.nan)
    hi = np.where(some, np.where(ok, rows, -np.inf).max(axis=0, initial=-np.inf), np.nan)
    mean = np.where(some, np.where(ok, rows, 0.0).sum(axis=0) / np.maximum(cnt, 1), np.nan)
    return lo, hi, mean


def _max_dev(d, mean):
    """(T, r) of max over r = 1..R of |d(r) - mean(r)| where both are defined; (NaN, 0) where none is."""
    dev = np.abs(d[1:] - mean[1:])
    if np.isnan(dev).all():
        return np.nan, 0
    k = int(np.nanargmax(dev))
    return float(dev[k]), k + 1


def analyse(n, pairs, pairs_all, A, N):
    """Counts [(1 + S), R + 1] -> the observed columns, the envelope, the global maximum-absolute-deviation test."""
    n, pairs, pairs_all = (np.asarray(v, np.int64) for v in (n, pairs, pairs_all))
    S = len(n) - 1
    cols = ripley_columns(n[0], pairs[0], pairs_all[0], A, N)
    sims = np.array([ripley_columns(n[s], pairs[s], pairs_all[s], A, N)["L_minus_r"] for s in range(1, S + 1)])
    sims = sims.reshape(S, n.shape[1])
    lo, hi, mean = envelope(sims)
    res = {**cols, "env_lo": lo, "env_hi": hi, "env_mean": mean, "csr_p": np.nan, "r_max_dev": 0, "max_dev": np.nan, "pattern": ""}
    d = cols["L_minus_r"]
    with np.errstate(invalid="ignore"):
        res["outside"] = np.where(d < lo, -1, np.where(d > hi, 1, 0)).astype(np.int64)
    if S == 0:
        return res
    T, r = _max_dev(d, mean)
    if np.isnan(T):
        return res
    Ts = np.array([_max_dev(row, mean)[0] for row in sims])
    res["csr_p"] = (1 + int((Ts >= T).sum())) / (S + 1)              # a NaN T_s compares False
    res["r_max_dev"], res["max_dev"] = r, T
    res["pattern"] = "random" if res["csr_p"] > ALPHA else "clustered" if d[r] > mean[r] else "regular"
    return res


def summary_row(filename, info, res):
    """The row of spatial_per_image.csv: info of droplet_points, res of analyse."""
    A, N = info["A"], info["N"]
    return {"filename": filename, "n_points": N, "n_dropped": info["n_dropped"], "window_px": A,
            "droplets_per_10k_px": 1e4 * N / A if A else np.nan, "csr_p": res["csr_p"], "r_max_dev": res["r_max_dev"],
            "max_dev": res["max_dev"], "pattern": res["pattern"]}


def table_rows(filename, counts, res, px_per_um=None):
    """The rows r = 1..R of spatial_stats.csv: counts = (n, pairs, pairs_all) as ripley_counts_numpy returns them."""
    n, pairs = counts[0][0], counts[1][0]
    rows = []
    for r in range(1, len(n)):
        row = {"filename": filename, "r_px": r}
        if px_per_um is not None:
            row["r_micron"] = r / px_per_um
        row.update({"n_eligible": int(n[r]), "pairs": int(pairs[r])})
        row.update({q: float(res[q][r]) for q in ("K", "L", "L_minus_r", "g", "K_raw", "env_lo", "env_hi", "env_mean")})
        row["outside"] = int(res["outside"][r])
        rows.append(row)
    return rows


def table_columns(px_per_um=None):
    return TABLE_COLUMNS if px_per_um is None else TABLE_COLUMNS[:2] + ("r_micron",) + TABLE_COLUMNS[2:]


def spatial_record(area, sum_y, sum_x, h, w, rmax, n_sim, seed, window=None):
    """The host record of one image, with the keys of spatial.spatial_stats_batch: py, px, N, n_dropped, A, n, pairs, pairs_all."""
    py, px, info = droplet_points(area, sum_y, sum_x, h, w, window)
    n, pairs, pairs_all = ripley_counts_numpy(py, px, h, w, rmax, n_sim, seed, window)
    return {"py": py, "px": px, **info, "n": n, "pairs": pairs, "pairs_all": pairs_all}
