"""Plain-loop restatement of the scaled crop rule (utils/crops.py:window_scaled / crop_gather_scaled_numpy,
csrc/crop.hip:crop_gather_scaled_kernel) and the fixtures its CPU and GPU tests share.  One output pixel at a time, with its own
taps and its own integer passes: nothing of utils.data_loader.resize_linear_cv2_u8, linear_tables, nearest_index, np.rot90 or
utils.tiling.fold.  Images, shapes and the unscaled restatement come from tests/crops_ref.py."""
import math

import numpy as np

from tests import crops_ref as cr

S = cr.S
TS = [16, 31, 32, 33, 47, 64]          # S / 2, one below / at / one above S, an odd ratio, 2 S


def axis_taps(d, T, s, is_x):
    """Lattice coordinate d of s -> ((i0, i1), (a0, a1)): two source indices inside 0..T-1 and their 11-bit weights."""
    f = (d + 0.5) * (T / s) - 0.5
    first = math.floor(f)
    frac = np.float32(f - first)
    a0, a1 = int(np.rint((np.float32(1.0) - frac) * np.float32(2048.0))), int(np.rint(frac * np.float32(2048.0)))
    if is_x:
        if first < 0 or first >= T - 1:                    # left of the first / at or right of the last pixel: one tap
            a0, a1 = 2048, 0
        i0 = min(max(first, 0), T - 1)
        return (i0, min(i0 + 1, T - 1)), (a0, a1)
    return (min(max(first, 0), T - 1), min(max(first + 1, 0), T - 1)), (a0, a1)        # two clamped taps, weights kept


def scaled_window_loops(img, mask, y0, x0, T, s):
    """The T x T window at (y0, x0) resampled to s x s -> (uint8 [s, s, C], uint8 [s, s]), pixel by pixel."""
    h, w, c = img.shape
    out, om = np.empty((s, s, c), np.uint8), np.empty((s, s), np.uint8)
    for ly in range(s):
        (ya, yb), (b0, b1) = axis_taps(ly, T, s, False)
        ra, rb = cr.fold_loop(y0 + ya, h), cr.fold_loop(y0 + yb, h)
        my = cr.fold_loop(y0 + min(math.floor(ly * (T / s)), T - 1), h)
        for lx in range(s):
            (xa, xb), (a0, a1) = axis_taps(lx, T, s, True)
            ca, cb = cr.fold_loop(x0 + xa, w), cr.fold_loop(x0 + xb, w)
            for ch in range(c):
                r0 = int(img[ra, ca, ch]) * a0 + int(img[ra, cb, ch]) * a1
                r1 = int(img[rb, ca, ch]) * a0 + int(img[rb, cb, ch]) * a1
                v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
                out[ly, lx, ch] = min(max(v, 0), 255)
            om[ly, lx] = mask[my, cr.fold_loop(x0 + min(math.floor(lx * (T / s)), T - 1), w)]
    return out, om


_SOURCE = {}


def source_index(s, p):
    """(fy [s, s], fx [s, s]): the lattice pixel every output pixel shows (crops_ref.source_loop, tabulated once per
    (s, k, hflip, vflip))."""
    key = (s, p["k"], bool(p["hflip"]), bool(p["vflip"]))
    if key not in _SOURCE:
        fy, fx = np.empty((s, s), np.int64), np.empty((s, s), np.int64)
        for y in range(s):
            for x in range(s):
                fy[y, x], fx[y, x] = cr.source_loop(y, x, s, p)
        _SOURCE[key] = (fy, fx)
    return _SOURCE[key]


def scaled_sample(win_u8, mwin, img_max_u8, s, p):
    """One sample without elastic from its restated lattice (scaled_window_loops): (out [C, s, s] float32, mask [1, s, s])."""
    fy, fx = source_index(s, p)
    v = win_u8[fy, fx].astype(np.float32) / np.float32(255.0)
    if p["bc"]:
        beta_max = np.float32(p["beta"] * float(np.float32(int(img_max_u8)) / np.float32(255.0)))
        v = (np.float32(p["alpha"]) * v).astype(np.float32) + beta_max
        v = np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))
    return np.ascontiguousarray(v.transpose(2, 0, 1)), mwin[fy, fx].astype(np.float32)[None]


def records(seed=1, bc_share=0.5, s=S, ts=TS):
    """Every image of crops_ref.SHAPES at the end origins of each source side of `ts`, with every k and both flips, brightness
    / contrast on about half: crops_ref.records with a ``T`` per record (67 windows x 16 = 1072 records at the defaults)."""
    r = np.random.default_rng(seed)
    recs = []
    for i, (h, w) in enumerate(cr.SHAPES):
        for T in ts:
            for y0, x0 in cr.end_origins(h, w, T):
                for k in range(4):
                    for hf in (False, True):
                        for vf in (False, True):
                            bc = bool(r.random() < bc_share)
                            recs.append(dict(img=i, y0=y0, x0=x0, T=T, params=cr.params(
                                hf, vf, k, bc, 1.0 + r.uniform(-0.2, 0.2) if bc else 1.0, r.uniform(-0.2, 0.2) if bc else 0.0)))
    return recs


# ---- unetdc_crop_gather_scaled calls that must be refused ------------------------------------------------------------------------
def _record(**kw):
    from unet_dc_segmentation_amd.crops import CROP_SCALED_DTYPE
    r = np.zeros(1, CROP_SCALED_DTYPE)
    r["h"], r["w"], r["field"], r["alpha"], r["t"] = 40, 56, -1, 1.0, S
    for k, v in kw.items():
        r[k] = v
    return r


# everything crops_ref.REFUSED holds (at t = S the origin ranges are the same), the origin range taken against t, and t itself
REFUSED = dict(cr.REFUSED)
REFUSED.update({
    "t below S / 2": (dict(t=15), dict()),
    "t above 2 S": (dict(t=65), dict()),
    "t = 0": (dict(t=0), dict()),
    "t negative": (dict(t=-32), dict()),
    "y0 past h - t": (dict(t=36, y0=5), dict()),                 # 5 <= 40 - 32: unetdc_crop_gather would accept it
    "x0 past w - t": (dict(t=48, x0=9), dict()),
    "y0 on an axis t folds": (dict(t=48, y0=1), dict()),          # 40 rows < 48
})


def refused_call(lib, name, ptrs):
    """crops_ref.refused_call for unetdc_crop_gather_scaled: a 40 x 56 x 3 image that exactly fills its buffers, S = 32, one
    record with t = 32 and the changes of REFUSED[name]."""
    rec_kw, call_kw = REFUSED[name]
    rec = _record(**rec_kw)
    a = dict(ptrs, S=S, c=3, records=rec.ctypes.data, nfields=0, fields=None)
    a.update(call_kw)
    return lib.unetdc_crop_gather_scaled(a["images"], 40 * 56 * a["c"] if a["c"] > 0 else 0, a["masks"], 40 * 56, a["c"], a["S"],
                                         a["records"], 1, a["fields"], a["nfields"], a["out_img"], a["out_mask"], None)
