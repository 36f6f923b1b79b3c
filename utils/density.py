"""Radial and spatial droplet density maps on the host: the analysis of the reference's ``quantify_pipline.py``
(generate_roi_mask :44-51, the ROI centroid :133-135, get_targets :61-91, density_maps :93-97, plt.imsave of the normalised
maps :141-142), restated on numpy.

cv2 is not available to this build: the OpenCV steps of the ROI (RGB2GRAY, the 8-bit GaussianBlur, Otsu, MORPH_CLOSE / OPEN)
are written out in integer arithmetic exactly as OpenCV defines them, as ``utils/data_loader.py`` does for the rolling ball
(parity against cv2 unpinned).  The spatial map calls ``scipy.ndimage.gaussian_filter`` itself.  This module is the CPU path of
``quantify_droplets_batch.py --density_maps`` and the yardstick of the HIP kernels (csrc/density.hip,
tests/test_gpu_density.py).
"""
from __future__ import annotations

import numpy as np

BLUR_K = 15                 # GaussianBlur((15, 15), 0) and the 15 x 15 morphology rectangle of generate_roi_mask
FLT_EPSILON = float(np.finfo(np.float32).eps)


def blur_taps_fixed(n=BLUR_K):
    """OpenCV's bit-exact 8-bit Gaussian kernel (getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED): sigma =
    0.15 n + 0.35 for sigma <= 0, taps exp(-(i - n//2)^2 / (2 sigma^2)) normalised, then 8 fractional bits by error diffusion
    from the outermost tap inwards (round half to even on tap * 256 + carried error); the centre tap is 256 minus the rest."""
    sigma = 0.15 * n + 0.35
    mid = n // 2
    k = np.exp(-((np.arange(n) - mid) ** 2) / (2.0 * sigma * sigma))
    k = k / k.sum()
    out = np.zeros(n, dtype=np.int64)
    err = 0.0
    for i in range(mid):
        adj = k[i] * 256.0 + err
        v = int(np.rint(adj))
        err = adj - v
        out[i] = out[n - 1 - i] = v
    out[mid] = 256 - 2 * int(out[:mid].sum())
    return out


BLUR_TAPS = blur_taps_fixed()


def rgb_to_gray(rgb):
    """cv2.cvtColor(RGB2GRAY) on uint8: (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    r, g, b = (rgb[..., c].astype(np.int32) for c in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def gaussian_blur_u8(gray, taps=BLUR_TAPS):
    """cv2.GaussianBlur(gray, (15, 15), 0) on uint8: separable fixed-point sums over a BORDER_REFLECT_101 border (numpy's
    mode "reflect"), out = (sum_i sum_j k_i k_j g + 32768) >> 16.  Exact integers (at most 255 * 2^16)."""
    r = len(taps) // 2
    h, w = gray.shape
    p = np.pad(gray.astype(np.int64), r, mode="reflect")
    rows = np.zeros((h + 2 * r, w), dtype=np.int64)
    for i, k in enumerate(taps):
        rows += int(k) * p[:, i:i + w]
    acc = np.zeros((h, w), dtype=np.int64)
    for j, k in enumerate(taps):
        acc += int(k) * rows[j:j + h]
    return ((acc + 32768) >> 16).astype(np.uint8)


def otsu_threshold(hist):
    """cv2.threshold(..., THRESH_BINARY | THRESH_OTSU)'s threshold from a 256-bin histogram: OpenCV's double-precision scan
    (Python floats are IEEE doubles and Python never fuses a multiply-add)."""
    hist = [int(v) for v in hist]
    scale = 1.0 / sum(hist)
    mu = 0.0
    for i in range(256):
        mu += i * float(hist[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    for i in range(256):
        p_i = hist[i] * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma = sigma
            max_val = i
    return max_val


def _window(a, k, op, ident, axis):
    """op over the k-window centred on every element along `axis` (anchor k // 2); elements outside the array do not take part."""
    r = k // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, k - 1 - r)
    p = np.pad(a, pad, mode="constant", constant_values=ident)
    return op(np.lib.stride_tricks.sliding_window_view(p, k, axis=axis), axis=-1)


def morph_rect(plane, k, is_max):
    """cv2.dilate (is_max) / cv2.erode of a uint8 plane with the k x k rectangle, anchor at the centre, pixels outside the image
    ignored (OpenCV's default morphology border).  A rectangle is separable: rows, then columns."""
    op, ident = (np.max, 0) if is_max else (np.min, 255)
    return _window(_window(plane, k, op, ident, 1), k, op, ident, 0).astype(np.uint8)


def roi_mask(rgb):
    """generate_roi_mask (quantify_pipline.py:44-51) -> (blurred uint8, Otsu threshold, roi uint8 {0, 1})."""
    blur = gaussian_blur_u8(rgb_to_gray(rgb))
    t = otsu_threshold(np.bincount(blur.ravel(), minlength=256))
    b = np.where(blur > t, 255, 0).astype(np.uint8)
    closed = morph_rect(morph_rect(b, BLUR_K, True), BLUR_K, False)              # MORPH_CLOSE
    opened = morph_rect(morph_rect(closed, BLUR_K, False), BLUR_K, True)         # MORPH_OPEN
    return blur, t, (opened > 0).astype(np.uint8)


def roi_centroid(roi):
    """cv2.moments(roi) -> (int(m10 / m00), int(m01 / m00), m00), (w // 2, h // 2) for an empty ROI (:133-135)."""
    h, w = roi.shape
    ys, xs = np.nonzero(roi)
    m00 = len(xs)
    if m00 == 0:
        return w // 2, h // 2, 0
    return int(float(xs.sum()) / m00), int(float(ys.sum()) / m00), m00


def droplet_centroids(mask):
    """(row, column) centroids of the 4-connected components of `mask`, no area filter, in label order: sum / area in float64."""
    from scipy import ndimage
    lbl, n = ndimage.label(mask)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    area = np.bincount(lbl.ravel(), minlength=n + 1)[1:].astype(np.float64)
    yy, xx = np.indices(mask.shape)
    sy = np.bincount(lbl.ravel(), weights=yy.ravel(), minlength=n + 1)[1:]
    sx = np.bincount(lbl.ravel(), weights=xx.ravel(), minlength=n + 1)[1:]
    return sy / area, sx / area


def ring_of(bounds, d):
    """Ring i with bounds[i] < d <= bounds[i + 1] for every value of d, -1 where there is none."""
    L = len(bounds) - 1
    i = np.searchsorted(bounds[:L], d, side="left") - 1
    ok = (i >= 0) & (d <= bounds[np.clip(i + 1, 0, L)])
    return np.where(ok, i, -1)


def radial_map(mask, roi, nb_layers, cy, cx, centroids=None):
    """get_targets (:61-91) -> (radial float32 map, ring index uint8 (i + 1 on ring i, 0 elsewhere), ring counts int64[L],
    largest ROI distance).  centroids: (rows, cols) of the droplets, default droplet_centroids(mask)."""
    cy_all, cx_all = droplet_centroids(mask) if centroids is None else centroids
    counts = np.zeros(nb_layers, dtype=np.int64)
    ring_idx = np.zeros(mask.shape, dtype=np.uint8)
    image = np.zeros(mask.shape, dtype=np.float32)
    ys, xs = np.nonzero(roi)
    if len(ys) == 0:
        return image, ring_idx, counts, 0.0
    d = np.sqrt((xs - cx) ** 2 + (ys - cy) ** 2)
    maxd = float(np.max(d))
    bounds = np.linspace(0, maxd, nb_layers + 1)
    ring = ring_of(bounds, d)
    ring_idx[ys, xs] = (ring + 1).astype(np.uint8)
    if len(cx_all):
        dc = np.sqrt((np.asarray(cx_all) - cx) ** 2 + (np.asarray(cy_all) - cy) ** 2)
        r = ring_of(bounds, dc)
        counts = np.bincount(r[r >= 0], minlength=nb_layers)[:nb_layers].astype(np.int64)
        image[ys, xs] = np.where(ring >= 0, counts[np.maximum(ring, 0)], 0).astype(np.float32)
    return image, ring_idx, counts, maxd


def spatial_map(mask, roi, kernel_size=21):
    """density_maps (:93-97): gaussian_filter(mask, k / 6) / (gaussian_filter(roi, k / 6) + 1e-5) * 100, float32."""
    from scipy.ndimage import gaussian_filter
    s = kernel_size / 6
    m = gaussian_filter(mask.astype(np.float32), sigma=s)
    m = m / (gaussian_filter(roi.astype(np.float32), sigma=s) + 1e-5)
    m *= 100
    return m


def gaussian_taps(sigma):
    """scipy.ndimage's Gaussian weights for truncate=4 (_gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5))), centre first: the
    host-computed fp64 taps the HIP kernel is given."""
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:], dtype=np.float64)


def colormap_index(m):
    """uint8 index into a 256-entry colormap of plt.imsave(normalize(m), cmap=...): normalize is (v - min) / (max - min) in
    float32 (the map unchanged if max == min, which imsave then maps to entry 0); the entry is min(int(t * 256), 255)."""
    m = np.asarray(m, dtype=np.float32)
    mn, mx = m.min(), m.max()
    if not mx > mn:
        return np.zeros(m.shape, dtype=np.uint8)
    t = (m - mn) / (mx - mn)
    return np.minimum((t * np.float32(256)).astype(np.int64), 255).astype(np.uint8)


_LUTS = {}


def colormap_lut(name="hot"):
    """[256, 4] uint8 RGBA table of a matplotlib colormap (plt.imsave's pixels are lut[colormap_index(map)])."""
    if name not in _LUTS:
        import matplotlib
        _LUTS[name] = np.ascontiguousarray(matplotlib.colormaps[name](np.arange(256), bytes=True))
    return _LUTS[name]


def density_maps(rgb, mask, nb_layers=10, kernel_size=21):
    """The whole analysis of one micrograph: rgb [h, w, 3] uint8 (decoded, before the rolling ball), mask [h, w] uint8 {0, 1}.
    Returns a dict with the intermediate planes, the per-image numbers and the two colormap index planes."""
    blur, t, roi = roi_mask(rgb)
    cx, cy, area = roi_centroid(roi)
    radial, ring, counts, maxd = radial_map(mask, roi, nb_layers, cy, cx)
    spatial = spatial_map(mask, roi, kernel_size)
    return {"blur": blur, "threshold": t, "roi": roi, "roi_area": area, "cx": cx, "cy": cy, "max_ring_distance": maxd,
            "ring_counts": counts, "ring": ring, "radial": radial, "spatial": spatial,
            "radial_index": colormap_index(radial), "spatial_index": colormap_index(spatial)}


def csv_row(filename, r, nb_layers):
    """One row of density_per_image.csv."""
    row = {"filename": filename, "roi_area_px": int(r["roi_area"]), "roi_centroid_x": int(r["cx"]),
           "roi_centroid_y": int(r["cy"]), "otsu_threshold": int(r["threshold"]),
           "max_ring_distance_px": float(r["max_ring_distance"])}
    for i in range(nb_layers):
        row[f"ring_{i + 1}"] = int(r["ring_counts"][i])
    return row


def write_pngs(radial_index, spatial_index, out_dir, name, cmap="hot"):
    """{name}_radial_density.png and {name}_spatial_density.png: RGBA pixels lut[index], the pixels plt.imsave writes.
    compress_level=1: the same pixels at about half the deflate time of PIL's default level 6 -- deflate is the slowest
    step of the density arm -- for larger files."""
    from PIL import Image
    lut = colormap_lut(cmap)
    Image.fromarray(lut[radial_index]).save(str(out_dir / f"{name}_radial_density.png"), compress_level=1)
    Image.fromarray(lut[spatial_index]).save(str(out_dir / f"{name}_spatial_density.png"), compress_level=1)


def ring_bounds(maxd, nb_layers):
    """np.linspace(0, maxd, L + 1) as the kernels form it: b_i = i * (maxd / L), b_L = maxd."""
    step = maxd / nb_layers
    return np.array([i * step for i in range(nb_layers)] + [maxd], dtype=np.float64)
