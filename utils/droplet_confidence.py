"""Per-droplet confidence and test-time-augmentation disagreement on the host (numpy only).  The definition is DESIGN.md
section 23; this module is the CPU path of quantify_droplets_batch.py --confidence and the yardstick of csrc/confidence.hip.
Every per-pixel quantity is an integer (a probability quantised to 16 bits, a table entry, a count), so sums, minima and maxima
do not depend on the order in which anything runs: the device result equals this one bit for bit."""
from __future__ import annotations

import numpy as np

QMAX = 65535
DEFAULT_BAND = 0.1          # a convention of the command line, not a measured number
MIN_INIT, MAX_INIT = np.iinfo(np.int64).max, -1
CONF_QUANTITIES = ("n", "Sq", "Sqq", "min_q", "max_q", "n_band", "Sh", "Sspread", "max_spread", "n_unstable")
ENVELOPE_QUANTITIES = ("Sspread", "max_spread", "n_unstable")         # keep their initial values without an envelope
IMAGE_QUANTITIES = ("n_px", "n_fg", "Sh_all", "Sh_fg", "n_band_all", "n_band_fg", "n_unstable_all", "Sspread_all")
IMAGE_COLUMNS = ("entropy_mean", "entropy_mean_bg", "uncertain_px", "uncertain_bg_px", "unstable_px", "tta_spread_mean", "droplets",
                 "min_droplet_prob_mean")


def check_band(band):
    """-> band as float; ValueError for what the stage refuses (a number in 0..0.5)."""
    if isinstance(band, bool) or not isinstance(band, (int, float, np.integer, np.floating)) or not 0 <= float(band) <= 0.5:
        raise ValueError(f"the uncertainty band must be a number in 0..0.5, not {band!r}")
    return float(band)


def quant(p):
    """Probabilities -> int64 in 0..65535: rint(float32(clamp(p, 0, 1)) * float32(65535)), the product in fp32, ties to even;
    a NaN becomes 0 (fmax / fmin return the other operand).  On the device __float2int_rn(__fmul_rn(fminf(fmaxf(p, 0), 1), 65535.f))."""
    c = np.fmin(np.fmax(np.asarray(p, dtype=np.float32), np.float32(0)), np.float32(1))
    return np.rint(c * np.float32(QMAX)).astype(np.int64)


_table = None


def entropy_table():
    """uint16 [65536]: H16[q] = rint(65535 * H2(q / 65535)) in float64, H2 the binary entropy in bits (0 at both ends).  No
    entry comes closer than 7.5e-7 to a rounding tie, so the table does not depend on the host's libm."""
    global _table
    if _table is None:
        p = np.arange(QMAX + 1, dtype=np.float64) / QMAX
        with np.errstate(divide="ignore", invalid="ignore"):
            h = -(p * np.log2(p) + (1.0 - p) * np.log2(1.0 - p))
        h[0] = h[QMAX] = 0.0
        _table = np.rint(QMAX * h).astype(np.uint16)
        _table.setflags(write=False)
    return _table


def sample_index(dst, src):
    """Source index of each destination index: min(floor(d * src / dst), src - 1), the rule of unetdc_mask_from_probs."""
    return np.minimum(np.floor(np.arange(dst) * (src / dst)).astype(np.int64), src - 1)


def _sums(index, values, size):
    """Exact int64 sums of non-negative `values` (below 2^32) per index: two float64 bincounts of 16-bit halves."""
    lo = np.bincount(index, weights=(values & 0xFFFF).astype(np.float64), minlength=size)
    hi = np.bincount(index, weights=(values >> 16).astype(np.float64), minlength=size)
    return (hi.astype(np.int64) << 16) + lo.astype(np.int64)


def confidence_numpy(labels, probs, thresh, band, lo=None, hi=None, max_out=None, maps=False):
    """labels: int [oh, ow] label map; probs (and the optional envelope lo, hi): fp32 [ph, pw] -> the record
    {every name of CONF_QUANTITIES: int64 [max_out] (entry k - 1 for droplet k; max_out = the largest label without one),
     "image": int64 [8] in the order of IMAGE_QUANTITIES, "envelope": whether lo / hi were given,
     "entropy_u8" / "spread_u8": uint8 [oh, ow] maps H16[q] >> 8 and spread >> 8 (None without maps; spread needs an envelope)}."""
    band = check_band(band)
    if (lo is None) != (hi is None):
        raise ValueError("the envelope is both lo and hi, or neither")
    lab = np.asarray(labels).astype(np.int64)
    probs = np.asarray(probs, dtype=np.float32)
    oh, ow = lab.shape
    ph, pw = probs.shape
    max_out = int(lab.max(initial=0)) if max_out is None else int(max_out)
    iy, ix = sample_index(oh, ph)[:, None], sample_index(ow, pw)[None, :]
    t32 = np.float32(thresh)
    q = quant(probs)[iy, ix]
    h16 = entropy_table()[q].astype(np.int64)
    in_band = np.abs(q - int(quant(t32))) <= int(quant(band))
    env = lo is not None
    if env:
        lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
        if lo.shape != probs.shape or hi.shape != probs.shape:
            raise ValueError("the envelope planes have the size of the probabilities")
        spread = (quant(hi) - quant(lo))[iy, ix]
        unstable = (~(lo > t32) & (hi > t32))[iy, ix]
    fg = lab > 0
    image = np.array([lab.size, fg.sum(), h16.sum(), h16[fg].sum(), in_band.sum(), (in_band & fg).sum(),
                      unstable.sum() if env else 0, spread.sum() if env else 0], dtype=np.int64)
    rec = {name: np.full(max_out, MIN_INIT if name.startswith("min_") else MAX_INIT if name.startswith("max_") else 0, np.int64)
           for name in CONF_QUANTITIES}
    sel = (lab >= 1) & (lab <= max_out)
    k, n = lab[sel] - 1, max_out
    if k.size:
        qs = q[sel]
        rec["n"] = np.bincount(k, minlength=n).astype(np.int64)
        rec["Sq"] = _sums(k, qs, n)
        rec["Sqq"] = _sums(k, qs * qs, n)
        np.minimum.at(rec["min_q"], k, qs)
        np.maximum.at(rec["max_q"], k, qs)
        rec["n_band"] = np.bincount(k[in_band[sel]], minlength=n).astype(np.int64)
        rec["Sh"] = _sums(k, h16[sel], n)
        if env:
            rec["Sspread"] = _sums(k, spread[sel], n)
            np.maximum.at(rec["max_spread"], k, spread[sel])
            rec["n_unstable"] = np.bincount(k[unstable[sel]], minlength=n).astype(np.int64)
    rec["image"], rec["envelope"] = image, env
    rec["entropy_u8"] = (h16 >> 8).astype(np.uint8) if maps else None
    rec["spread_u8"] = (spread >> 8).astype(np.uint8) if maps and env else None
    return rec


def confidence_columns(rec):
    """The float64 columns --confidence adds to a droplet table: prob_mean, prob_std, prob_min, prob_max, entropy_mean (bits),
    uncertain_frac; with an envelope tta_spread_mean, tta_spread_max, unstable_frac.  A droplet without pixels gets NaN."""
    v = {name: np.asarray(rec[name], dtype=np.int64).astype(np.float64) for name in CONF_QUANTITIES}
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(v["n"] > 0, v["n"], np.nan)
        mean = v["Sq"] / n
        out = {"prob_mean": v["Sq"] / (QMAX * n),
               "prob_std": np.sqrt(np.maximum(v["Sqq"] / n - mean * mean, 0.0)) / QMAX,
               "prob_min": v["min_q"] / QMAX + 0.0 * n, "prob_max": v["max_q"] / QMAX + 0.0 * n,
               "entropy_mean": v["Sh"] / (QMAX * n), "uncertain_frac": v["n_band"] / n}
        if rec.get("envelope"):
            out.update({"tta_spread_mean": v["Sspread"] / (QMAX * n), "tta_spread_max": v["max_spread"] / QMAX + 0.0 * n,
                        "unstable_frac": v["n_unstable"] / n})
    return out


def image_columns(rec):
    """One image's row of confidence_per_image.csv (without the file name), in the order of IMAGE_COLUMNS: the mean entropy in
    bits over all pixels and over the background, uncertain pixels in all and on the background (the missed-droplet indicator),
    with an envelope the unstable pixels and the mean spread (NaN without), the droplets and their smallest prob_mean."""
    im = dict(zip(IMAGE_QUANTITIES, (int(x) for x in rec["image"])))
    n_bg = im["n_px"] - im["n_fg"]
    env = bool(rec.get("envelope"))
    means = confidence_columns(rec)["prob_mean"]
    means = means[np.isfinite(means)]
    return {"entropy_mean": im["Sh_all"] / (QMAX * im["n_px"]),
            "entropy_mean_bg": (im["Sh_all"] - im["Sh_fg"]) / (QMAX * n_bg) if n_bg else float("nan"),
            "uncertain_px": im["n_band_all"], "uncertain_bg_px": im["n_band_all"] - im["n_band_fg"],
            "unstable_px": im["n_unstable_all"] if env else float("nan"),
            "tta_spread_mean": im["Sspread_all"] / (QMAX * im["n_px"]) if env else float("nan"),
            "droplets": int(np.count_nonzero(np.asarray(rec["n"]) > 0)),
            "min_droplet_prob_mean": float(means.min()) if means.size else float("nan")}
