"""An independent restatement of the confidence rule for the tests: plain loops over the labels with
boolean masks and Python integers, scalar arithmetic for the quantisation and the entropy.  Slow; only for small fixtures."""
import math
import struct

import numpy as np

NAMES = ("n", "Sq", "Sqq", "min_q", "max_q", "n_band", "Sh", "Sspread", "max_spread", "n_unstable")
IMAGE_NAMES = ("n_px", "n_fg", "Sh_all", "Sh_fg", "n_band_all", "n_band_fg", "n_unstable_all", "Sspread_all")
INT64_MAX = 2 ** 63 - 1


def f32(x):
    """The nearest fp32 of a Python float, as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def quant_ref(p):
    """One probability -> 0..65535.  The product of two fp32 values is exact in a double (48 significant bits), so rounding it
    once to fp32 is the fp32 product; Python's round() is half to even."""
    p = float(p)
    if p != p or p < 0.0:
        p = 0.0
    p = 1.0 if p > 1.0 else f32(p)
    return int(round(f32(p * 65535.0)))


def entropy16_ref(q):
    if q == 0 or q == 65535:
        return 0
    p = q / 65535.0
    return int(round(65535.0 * -(p * math.log2(p) + (1.0 - p) * math.log2(1.0 - p))))


def source(d, dst, src):
    return min(int(math.floor(d * (src / dst))), src - 1)


def confidence_ref(labels, probs, thresh, band, lo=None, hi=None, max_out=None):
    labels = np.asarray(labels)
    oh, ow = labels.shape
    ph, pw = np.shape(probs)
    max_out = int(labels.max(initial=0)) if max_out is None else max_out
    t = f32(thresh)
    qt, bq = quant_ref(t), quant_ref(band)
    q = np.zeros((oh, ow), object)
    h = np.zeros((oh, ow), object)
    spread = np.zeros((oh, ow), object)
    inband = np.zeros((oh, ow), bool)
    unstable = np.zeros((oh, ow), bool)
    for y in range(oh):
        sy = source(y, oh, ph)
        for x in range(ow):
            sx = source(x, ow, pw)
            q[y, x] = quant_ref(probs[sy][sx])
            h[y, x] = entropy16_ref(q[y, x])
            inband[y, x] = abs(q[y, x] - qt) <= bq
            if lo is not None:
                a, b = float(lo[sy][sx]), float(hi[sy][sx])
                spread[y, x] = quant_ref(b) - quant_ref(a)
                unstable[y, x] = (not a > t) and b > t
    rows = {name: [INT64_MAX if name.startswith("min_") else -1 if name.startswith("max_") else 0] * max_out for name in NAMES}
    for k in range(1, max_out + 1):
        m = labels == k
        if not m.any():
            continue
        qs = [int(v) for v in q[m]]
        rows["n"][k - 1] = len(qs)
        rows["Sq"][k - 1] = sum(qs)
        rows["Sqq"][k - 1] = sum(v * v for v in qs)
        rows["min_q"][k - 1], rows["max_q"][k - 1] = min(qs), max(qs)
        rows["n_band"][k - 1] = int(inband[m].sum())
        rows["Sh"][k - 1] = sum(int(v) for v in h[m])
        if lo is not None:
            sp = [int(v) for v in spread[m]]
            rows["Sspread"][k - 1], rows["max_spread"][k - 1] = sum(sp), max(sp)
            rows["n_unstable"][k - 1] = int(unstable[m].sum())
    fg = labels > 0
    image = [labels.size, int(fg.sum()), sum(int(v) for v in h.ravel()), sum(int(v) for v in h[fg]), int(inband.sum()),
             int((inband & fg).sum()), int(unstable.sum()), sum(int(v) for v in spread.ravel())]
    return rows, dict(zip(IMAGE_NAMES, image)), (np.array(h, np.int64) >> 8).astype(np.uint8), (np.array(spread, np.int64) >> 8).astype(np.uint8)
