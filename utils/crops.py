"""Training at native resolution: random S x S windows of images kept at their own size.

This is the ONE statement of the rule: where a window lies (``draw_crop``), what it holds (``window``), what the training
sample made of it is (``crop_gather_numpy``, the host path of ``unetdc_crop_gather`` in csrc/crop.hip: same values, same order
of the float32 operations) and which windows an evaluation visits (``eval_plan``).  Only numpy is needed (scipy for a sample
that draws the elastic step).

Scale jitter and foreground-aware windows (``--crop_scale``, ``--crop_fg``) are stated here too: which side T a window has
(``t_range``), where it lies (``draw_crop_fg``), what it holds once resampled to S x S (``window_scaled``: the resized path's
own 8-bit rules, imported from utils.data_loader and unet_dc_segmentation_amd.droplets when first used) and the sample made
of it (``crop_gather_scaled_numpy``, the host path of ``unetdc_crop_gather_scaled``).
"""
import numpy as np

from utils.tiling import fold, tile_plan

MIN_CROP, MAX_CROP = 32, 1024        # --crop: a multiple of 16 (the network's rule) up to the largest elastic-field side
MIN_SCALE, MAX_SCALE = 0.5, 2.0      # --crop_scale LO HI: MIN_SCALE <= LO <= 1 <= HI <= MAX_SCALE
SCALE_DUST = 1e-9                    # 0.55 * 400 is 220.00000000000003 in double: the dust is taken off before ceil / floor


def check_crop(S):
    S = int(S)
    if S % 16 or not MIN_CROP <= S <= MAX_CROP:
        raise ValueError(f"crop size {S}: a multiple of 16 in {MIN_CROP}..{MAX_CROP}")
    return S


def sample_number(index, rep, R):
    """q = index * R + rep: `index` is the image's index in the whole training split, rep in 0..R-1 (--crops_per_image R)."""
    if not 0 <= int(rep) < int(R):
        raise ValueError(f"rep {rep} outside 0..{int(R) - 1}")
    return int(index) * int(R) + int(rep)


def draw_crop(seed, epoch, q, h, w, S):
    """(y0, x0) of sample q's window in an h x w image: y0 uniform over the integers 0..max(h - S, 0), then x0 over
    0..max(w - S, 0), from np.random.default_rng([seed, epoch, q, 1]).  The four-element key keeps this stream apart from
    augment.draw_params' [seed, epoch, q]; nothing depends on batch size, world size or worker count."""
    rng = np.random.default_rng([int(seed), int(epoch), int(q), 1])
    y0 = int(rng.integers(0, max(int(h) - int(S), 0) + 1))
    x0 = int(rng.integers(0, max(int(w) - int(S), 0) + 1))
    return y0, x0


def check_scale(scale):
    """(LO, HI) of --crop_scale as floats; ValueError unless MIN_SCALE <= LO <= 1 <= HI <= MAX_SCALE."""
    lo, hi = (float(v) for v in scale)
    if not (MIN_SCALE <= lo <= 1.0 <= hi <= MAX_SCALE):
        raise ValueError(f"crop scale ({lo}, {hi}): {MIN_SCALE} <= LO <= 1 <= HI <= {MAX_SCALE}")
    return lo, hi


def t_range(S, scale):
    """(Tlo, Thi): the source sides a window of crop size S may have under scale = (LO, HI): Tlo = ceil(LO * S - SCALE_DUST),
    Thi = floor(HI * S + SCALE_DUST), the ONE rounding of the two products (0.55 * 40 gives 22 and 0.55 * 400 gives 220, not 221).  Tlo <= S <= Thi,
    both within S / 2 .. 2 S (the limits of unetdc_crop_gather_scaled)."""
    lo, hi = check_scale(scale)
    return int(np.ceil(lo * int(S) - SCALE_DUST)), int(np.floor(hi * int(S) + SCALE_DUST))


def draw_crop_fg_branch(seed, epoch, q, h, w, S, scale=None, p_fg=0.0, fg=None):
    """draw_crop_fg and whether the window took the foreground branch: (y0, x0, T, took_fg)."""
    h, w, S, p_fg = int(h), int(w), int(S), float(p_fg)
    if not 0.0 <= p_fg <= 1.0:
        raise ValueError(f"p_fg {p_fg} outside [0, 1]")
    if p_fg > 0.0 and fg is None:
        raise ValueError("p_fg > 0 needs the image's foreground indices (np.flatnonzero(mask) as int32)")
    rng = np.random.default_rng([int(seed), int(epoch), int(q), 2])
    T = S
    if scale is not None:
        tlo, thi = t_range(S, scale)
        T = int(rng.integers(tlo, thi + 1))
    u = float(rng.random())
    ymax, xmax = max(h - T, 0), max(w - T, 0)
    if u < p_fg and len(fg) > 0:
        py, px = divmod(int(fg[int(rng.integers(0, len(fg)))]), w)
        oy, ox = int(rng.integers(0, T)), int(rng.integers(0, T))
        return min(max(py - oy, 0), ymax), min(max(px - ox, 0), xmax), T, True
    y0 = int(rng.integers(0, ymax + 1))
    x0 = int(rng.integers(0, xmax + 1))
    return y0, x0, T, False


def draw_crop_fg(seed, epoch, q, h, w, S, scale=None, p_fg=0.0, fg=None):
    """(y0, x0, T) of sample q's window under scale jitter and foreground-aware placement, from
    np.random.default_rng([seed, epoch, q, 2]) (draw_crop's [.., 1] and augment.draw_params' [seed, epoch, q] are other
    streams).  The draws, in this order:

    1. T = S if scale is None, else uniform over the integers of t_range(S, scale).
    2. u = rng.random(); the foreground branch is taken iff u < p_fg and len(fg) > 0.
    3. foreground branch: j uniform over 0..len(fg)-1, (py, px) = divmod(fg[j], w); oy, then ox, uniform over 0..T-1;
       y0 = min(max(py - oy, 0), max(h - T, 0)) and x0 likewise.
    4. otherwise y0 uniform over 0..max(h - T, 0), then x0 over 0..max(w - T, 0).

    fg: the raster indices of the mask's non-zero pixels as int32 (np.flatnonzero).  On an axis with dim >= T the chosen
    pixel lies inside [y0, y0 + T): py - oy <= py, and the clamp to dim - T keeps py < y0 + T because py <= dim - 1; on a
    folded axis the origin is 0 and the window covers the whole image.  Nothing depends on batch size, world size or worker
    count."""
    return draw_crop_fg_branch(seed, epoch, q, h, w, S, scale, p_fg, fg)[:3]


def image_max(img_u8):
    """The maximum of a cached uint8 image on the [0, 1] scale, float32(max) / float32(255) as a Python float: the
    ``float(img.max())`` of the resized path's brightness / contrast step."""
    img_u8 = np.asarray(img_u8)
    return float(np.float32(img_u8.max() if img_u8.size else 255) / np.float32(255.0))


def _window_u8(img, mask, y0, x0, S):
    """The S x S window as uint8: (img [S, S, C], mask [S, S]) of the pixels (fold(y0 + y, h), fold(x0 + x, w))."""
    img, mask = np.asarray(img), np.asarray(mask)
    if img.dtype != np.uint8 or img.ndim != 3 or mask.dtype != np.uint8 or mask.shape != img.shape[:2]:
        raise ValueError("window needs an [h, w, C] uint8 image and its [h, w] uint8 mask")
    h, w = mask.shape
    if not (0 <= y0 <= max(h - S, 0) and 0 <= x0 <= max(w - S, 0)):
        raise ValueError(f"origin ({y0}, {x0}) outside 0..{max(h - S, 0)}, 0..{max(w - S, 0)}")
    r = np.arange(S)
    ys, xs = fold(y0 + r, h), fold(x0 + r, w)
    return img[ys][:, xs], mask[ys][:, xs]


def window(img, mask, y0, x0, S):
    """img [h, w, C] uint8, mask [h, w] uint8 -> (win [S, S, C] float32 = float32(pixel) / 255.0f, mwin [S, S] uint8) of the
    pixels (fold(y0 + y, h), fold(x0 + x, w)).  Only an image smaller than S along an axis is folded."""
    win, mwin = _window_u8(img, mask, y0, x0, S)
    return win.astype(np.float32) / np.float32(255.0), mwin


def window_scaled(img, mask, y0, x0, T, S):
    """The T x T window at (y0, x0) (window's rule with T in place of S, as uint8) resampled to S x S -> (win [S, S, C]
    float32, mwin [S, S] uint8).  Image: utils.data_loader.resize_linear_cv2_u8 (OpenCV's 8-bit INTER_LINEAR, the taps of
    linear_tables(T, S)), then float32 / 255.0f; mask: unet_dc_segmentation_amd.droplets.resize_nearest_cv2 (nearest_index(S,
    T)): the rules the resized path applies to whole images.  resize_linear_cv2_u8 treats the axes differently at the border
    (x: one tap of weight 2048, y: two clamped taps), so the resize acts in the window's own orientation, before any flip or
    rotation.  At T == S it is the identity."""
    from unet_dc_segmentation_amd.droplets import resize_nearest_cv2
    from utils.data_loader import resize_linear_cv2_u8
    T, S = int(T), int(S)
    if not S <= 2 * T <= 4 * S:
        raise ValueError(f"source side {T} outside {(S + 1) // 2}..{2 * S}")
    src, srcmask = _window_u8(img, mask, y0, x0, T)
    win = resize_linear_cv2_u8(np.ascontiguousarray(src), S, S).astype(np.float32) / np.float32(255.0)
    return win, resize_nearest_cv2(np.ascontiguousarray(srcmask), S, S)


def crop_gather_numpy(images, masks, records, S, fields=None):
    """The training samples of `records` in float32 numpy -> (out_img [n, C, S, S], out_mask [n, 1, S, S]).

    images / masks: lists of [h, w, C] uint8 images and [h, w] uint8 {0, 1} masks (sizes may differ between images).
    records: one dict per sample with ``img`` (index into the lists), ``y0``, ``x0`` and ``params`` (an augment.draw_params
    record: hflip, vflip, k, bc, alpha, beta, elastic).  fields: per record None or (dx, dy), the S x S displacement fields
    of a sample that draws elastic.

    Each sample is TrainAugment's random part applied to the window as if it were the image -- hflip, vflip, rot90(k),
    clip(alpha * win + beta_max, 0, 1), elastic -- with ONE deviation: beta_max = float32(beta * image_max(whole image)),
    not the window's own maximum (the device would need a reduction and a host wait per batch for that)."""
    return _gather_numpy(images, masks, records, S, fields, lambda img, mask, rec: window(img, mask, rec["y0"], rec["x0"], S))


def crop_gather_scaled_numpy(images, masks, records, S, fields=None):
    """crop_gather_numpy with window_scaled in place of window: every record carries its source side ``T`` too.  Everything
    after the window is unchanged: flips, rot90, brightness / contrast with the whole image's maximum, and the elastic step on
    the S x S lattice reflected at the window's border.  The host path of unetdc_crop_gather_scaled."""
    return _gather_numpy(images, masks, records, S, fields,
                         lambda img, mask, rec: window_scaled(img, mask, rec["y0"], rec["x0"], rec["T"], S))


def _gather_numpy(images, masks, records, S, fields, cut):
    S = int(S)
    c = np.shape(images[0])[2] if len(images) else 0
    out_img = np.empty((len(records), c, S, S), np.float32)
    out_mask = np.empty((len(records), 1, S, S), np.float32)
    for i, rec in enumerate(records):
        p = rec["params"]
        img, mask = cut(images[rec["img"]], masks[rec["img"]], rec)
        if p["hflip"]:
            img, mask = img[:, ::-1], mask[:, ::-1]
        if p["vflip"]:
            img, mask = img[::-1], mask[::-1]
        if p["k"]:
            img, mask = np.rot90(img, p["k"], (0, 1)), np.rot90(mask, p["k"], (0, 1))
        if p["bc"]:
            beta_max = np.float32(p["beta"] * image_max(images[rec["img"]]))             # the product formed in double
            img = np.clip(np.float32(p["alpha"]) * img + beta_max, np.float32(0.0), np.float32(1.0)).astype(np.float32)
        if p["elastic"]:
            from scipy import ndimage
            dx, dy = fields[i]
            yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
            coords = [yy + dy, xx + dx]
            img = np.ascontiguousarray(img)
            img = np.stack([ndimage.map_coordinates(img[..., ch], coords, order=1, mode="reflect")
                            for ch in range(img.shape[2])], axis=-1).astype(np.float32)
            mask = ndimage.map_coordinates(np.ascontiguousarray(mask), coords, order=0, mode="reflect").astype(np.uint8)
        out_img[i] = img.transpose(2, 0, 1)
        out_mask[i, 0] = mask
    return out_img, out_mask


def eval_plan(h, w, S):
    """[(y0, x0)] of the windows an evaluation visits, row-major: utils.tiling.tile_plan(h, w, S, 0), no augmentation.  The
    windows cover every pixel; where evenly spread windows overlap, a pixel is counted by each window that covers it."""
    yo, xo = tile_plan(h, w, S, 0)
    return [(y0, x0) for y0 in yo for x0 in xo]
