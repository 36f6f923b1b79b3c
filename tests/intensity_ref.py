"""Plain-loop restatement of DESIGN.md section 29 (ranks, window, projection), written from that section alone: sort the values,
index the sorted list.  The yardstick of utils/intensity_window.py (tests/test_intensity_cpu.py) and, through it and directly,
of csrc/window.hip (tests/test_gpu_intensity.py).  Also the value sets and rank lists both test files share."""
import functools

import numpy as np

PPM = 10 ** 6


def ranks_ref(arr, ppm):
    """uint16 [h][w][c] -> (value, below, equal) as lists [c][nq] of Python integers."""
    h, w, c = arr.shape
    n = h * w
    value, below, equal = [], [], []
    for ch in range(c):
        s = sorted(int(v) for v in arr[:, :, ch].ravel())
        vs, bs, es = [], [], []
        for p in ppm:
            k = (p * n + PPM - 1) // PPM                 # ceil(p n / 10^6) in integers
            if k < 1:
                k = 1
            v = s[k - 1]
            b = e = 0
            for x in s:
                if x < v:
                    b += 1
                elif x == v:
                    e += 1
            vs.append(v)
            bs.append(b)
            es.append(e)
        value.append(vs)
        below.append(bs)
        equal.append(es)
    return value, below, equal


def ranks_ref_fast(arr, ppm):
    """The same integers for the large shapes, where the double loop above would take minutes: sort, index, and count with two
    binary searches on the sorted list (bisect).  tests/test_intensity_cpu.py holds it against ranks_ref on the small sets."""
    import bisect
    h, w, c = arr.shape
    n = h * w
    out = ([], [], [])
    for ch in range(c):
        s = np.sort(arr[:, :, ch], axis=None).tolist()
        rows = ([], [], [])
        for p in ppm:
            k = max(1, (p * n + PPM - 1) // PPM)
            v = s[k - 1]
            lo, hi = bisect.bisect_left(s, v), bisect.bisect_right(s, v)
            for r, x in zip(rows, (v, lo, hi - lo)):
                r.append(x)
        for o, r in zip(out, rows):
            o.append(r)
    return out


def window_value(v, lo, hi):
    """One value through the window; levels outside 0..65535 are clamped to it first."""
    lo, hi = min(max(lo, 0), 65535), min(max(hi, 0), 65535)
    d = hi - lo
    if d <= 0:
        return 0
    t = min(max(v, lo), hi) - lo
    return (510 * t + d) // (2 * d)


def window_ref(arr, levels, dc):
    """uint16 [h][w][c], levels [c][2] -> uint8 [h][w][dc]; a 65536-entry table per channel stands for the per-pixel loop."""
    h, w, c = arr.shape
    assert dc == c or (dc == 3 and c == 1)
    out = np.zeros((h, w, dc), np.uint8)
    for ch in range(c):
        lo, hi = int(levels[ch][0]), int(levels[ch][1])
        present = np.unique(arr[:, :, ch])
        table = np.zeros(65536, np.uint8)
        for v in present.tolist():
            table[v] = window_value(v, lo, hi)
        if dc == c:
            out[:, :, ch] = table[arr[:, :, ch]]
        else:
            for k in range(3):
                out[:, :, k] = table[arr[:, :, 0]]
    return out


def planes_max_ref(planes):
    out = planes[0].copy()
    for p in range(1, planes.shape[0]):
        out = np.where(planes[p] > out, planes[p], out)
    return out


# ---- value sets (name -> uint16 [h, w, c]) and rank lists --------------------------------------------------------------------

VALUE_SETS = ("equal", "two", "one_bin", "edge_low", "edge_high", "ends", "ties", "micrograph", "uniform")
RANK_LISTS = {
    "min": [0],
    "max": [PPM],
    "five": [0, 1000, 500000, 999000, PPM],
    "repeat": [999000, 500000, 1000, 500000, 0],
    "eight": [0, 1, 250000, 500000, 500001, 750000, 999999, PPM],
}


def micrograph(h, w, seed=0):
    """A smooth 12-bit image: a slow background gradient, blobs and a little noise, 0..4095."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = 300.0 + 400.0 * yy / max(h - 1, 1) + 200.0 * xx / max(w - 1, 1)
    for _ in range(max(3, h * w // 20000)):
        cy, cx, r, a = rng.integers(0, h), rng.integers(0, w), rng.integers(3, 4 + max(h, w) // 8), rng.integers(500, 3200)
        img += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * r * r))
    img += rng.normal(0, 12, (h, w))
    return np.clip(np.rint(img), 0, 4095).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def value_set(name, h, w, c, seed=0):
    """Read-only uint16 [h, w, c]; the channels differ so that a channel mix-up shows."""
    rng = np.random.default_rng([seed, VALUE_SETS.index(name), h, w, c])
    n = h * w
    out = np.zeros((h, w, c), np.uint16)
    for ch in range(c):
        if name == "equal":
            a = np.full(n, 1234 + 257 * ch)
        elif name == "two":
            a = np.where(rng.random(n) < 0.3, 40000 + ch, 17 + ch)
        elif name == "one_bin":                          # one high byte: pass B decides everything
            a = (0x2A + ch) * 256 + rng.integers(0, 256, n)
        elif name == "edge_low":                         # 0x00FF / 0x0100 with neighbours on both sides
            a = rng.choice([0x00FD, 0x00FE, 0x00FF, 0x0100, 0x0101], n, p=[0.1, 0.15, 0.25, 0.3, 0.2])
        elif name == "edge_high":                        # 0xFEFF / 0xFF00
            a = rng.choice([0xFEFE, 0xFEFF, 0xFF00, 0xFF01, 0xFFFF], n, p=[0.2, 0.3, 0.25, 0.15, 0.1])
        elif name == "ends":                             # 0 and 65535 present, 65535 repeated
            a = rng.integers(0, 65536, n)
            a[rng.random(n) < 0.05] = 65535
            a[rng.integers(0, n)] = 0
            a[rng.integers(0, n)] = 65535
        elif name == "ties":                             # 60 % of the pixels hold the median value
            a = rng.integers(0, 65536, n)
            a[rng.random(n) < 0.6] = 0x8000 + ch
        elif name == "micrograph":
            a = micrograph(h, w, seed + ch).ravel()
        else:
            a = rng.integers(0, 65536, n)
        out[:, :, ch] = np.asarray(a).reshape(h, w)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ranks_of(name, h, w, c, ranks):
    """The restatement's answer for value_set(name, h, w, c) and RANK_LISTS[ranks], computed once: int32 [3, c, nq]."""
    arr = value_set(name, h, w, c)
    fn = ranks_ref if h * w <= 4096 else ranks_ref_fast
    out = np.asarray(fn(arr, RANK_LISTS[ranks]), np.int32)
    out.setflags(write=False)
    return out
