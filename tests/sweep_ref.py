"""Slow restatement of the threshold sweep, written from DESIGN.md section 14 alone: per output pixel, the K masks of the
grid evaluated one threshold after the other and counted.  It uses no monotonicity and no level shortcut, and carries its own
copy of the nearest index rule and of the 8-bit bilinear formula (nothing of utils/ or of the package is imported)."""
import math

import numpy as np


def grid_ref(K):
    """t_k = (float)k / (float)K: one fp32 division per threshold."""
    return [np.float32(k) / np.float32(K) for k in range(K)]


def nearest_index_ref(dst, src):
    """cv2's INTER_NEAREST: min(floor(d * (src / dst)), src - 1), in double."""
    scale = float(src) / float(dst)
    return [min(int(math.floor(d * scale)), src - 1) for d in range(dst)]


def linear_taps_ref(dst, src, clamp_weights):
    """OpenCV's 8-bit INTER_LINEAR per destination index: (first tap, second tap, weight of the first, of the second), 11-bit
    weights from the fp32 fraction.  x direction (clamp_weights): a first tap left of the first or at / right of the last
    source pixel is one tap of weight 2048.  y direction: the taps are clamped, the weights stay."""
    scale = float(src) / float(dst)
    out = []
    for d in range(dst):
        f = (d + 0.5) * scale - 0.5
        s = int(math.floor(f))
        f = np.float32(f - s)
        w0, w1 = int(np.rint(np.float32(np.float32(1.0) - f) * np.float32(2048))), int(np.rint(f * np.float32(2048)))
        if clamp_weights:
            if s < 0 or s >= src - 1:
                w0, w1 = 2048, 0
            s0 = min(max(s, 0), src - 1)
            s1 = min(s0 + 1, src - 1)
        else:
            s0, s1 = min(max(s, 0), src - 1), min(max(s + 1, 0), src - 1)
        out.append((s0, s1, w0, w1))
    return out


def sweep_ref(probs2d, gt, out_hw, K, linear):
    """-> int64 [2][K + 1]: hist[g][l] = pixels of class g = (gt != 0) that are set at exactly l thresholds of the grid."""
    p = np.asarray(probs2d, dtype=np.float32)
    ph, pw = p.shape
    oh, ow = out_hw
    g = np.asarray(gt)
    assert g.shape == (oh, ow)
    t = np.array(grid_ref(K), dtype=np.float32)
    hist = np.zeros((2, K + 1), np.int64)
    identity = (ph, pw) == (oh, ow)
    if linear and not identity:
        ys, xs = linear_taps_ref(oh, ph, False), linear_taps_ref(ow, pw, True)
    else:
        ys, xs = nearest_index_ref(oh, ph), nearest_index_ref(ow, pw)
    with np.errstate(invalid="ignore"):
        for y in range(oh):
            for x in range(ow):
                if linear and not identity:
                    y0, y1, b0, b1 = ys[y]
                    x0, x1, a0, a1 = xs[x]
                    # the K masks side by side (a vector over k); a NaN compares false
                    m00, m01 = (p[y0, x0] > t).astype(np.int64), (p[y0, x1] > t).astype(np.int64)
                    m10, m11 = (p[y1, x0] > t).astype(np.int64), (p[y1, x1] > t).astype(np.int64)
                    r0, r1 = m00 * a0 + m01 * a1, m10 * a0 + m11 * a1
                    v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
                    level = int(np.count_nonzero(np.clip(v, 0, 255)))
                else:
                    level = int(np.count_nonzero(p[ys[y], xs[x]] > t))
                hist[1 if g[y, x] != 0 else 0, level] += 1
    return hist
