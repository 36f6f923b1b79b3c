"""Training at native resolution: random S x S windows of images kept at their own size.

This is the ONE statement of the rule: where a window lies (``draw_crop``), what it holds (``window``), what the training
sample made of it is (``crop_gather_numpy``, the host path of ``unetdc_crop_gather`` in csrc/crop.hip: same values, same order
of the float32 operations) and which windows an evaluation visits (``eval_plan``).  Only numpy is needed (scipy for a sample
that draws the elastic step).
"""
import numpy as np

from utils.tiling import fold, tile_plan

MIN_CROP, MAX_CROP = 32, 1024        # --crop: a multiple of 16 (the network's rule) up to the largest elastic-field side


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


def image_max(img_u8):
    """The maximum of a cached uint8 image on the [0, 1] scale, float32(max) / float32(255) as a Python float: the
    ``float(img.max())`` of the resized path's brightness / contrast step."""
    img_u8 = np.asarray(img_u8)
    return float(np.float32(img_u8.max() if img_u8.size else 255) / np.float32(255.0))


def window(img, mask, y0, x0, S):
    """img [h, w, C] uint8, mask [h, w] uint8 -> (win [S, S, C] float32 = float32(pixel) / 255.0f, mwin [S, S] uint8) of the
    pixels (fold(y0 + y, h), fold(x0 + x, w)).  Only an image smaller than S along an axis is folded."""
    img, mask = np.asarray(img), np.asarray(mask)
    if img.dtype != np.uint8 or img.ndim != 3 or mask.dtype != np.uint8 or mask.shape != img.shape[:2]:
        raise ValueError("window needs an [h, w, C] uint8 image and its [h, w] uint8 mask")
    h, w = mask.shape
    if not (0 <= y0 <= max(h - S, 0) and 0 <= x0 <= max(w - S, 0)):
        raise ValueError(f"origin ({y0}, {x0}) outside 0..{max(h - S, 0)}, 0..{max(w - S, 0)}")
    r = np.arange(S)
    ys, xs = fold(y0 + r, h), fold(x0 + r, w)
    win = img[ys][:, xs].astype(np.float32) / np.float32(255.0)
    return win, mask[ys][:, xs]


def crop_gather_numpy(images, masks, records, S, fields=None):
    """The training samples of `records` in float32 numpy -> (out_img [n, C, S, S], out_mask [n, 1, S, S]).

    images / masks: lists of [h, w, C] uint8 images and [h, w] uint8 {0, 1} masks (sizes may differ between images).
    records: one dict per sample with ``img`` (index into the lists), ``y0``, ``x0`` and ``params`` (an augment.draw_params
    record: hflip, vflip, k, bc, alpha, beta, elastic).  fields: per record None or (dx, dy), the S x S displacement fields
    of a sample that draws elastic.

    Each sample is TrainAugment's random part applied to the window as if it were the image -- hflip, vflip, rot90(k),
    clip(alpha * win + beta_max, 0, 1), elastic -- with ONE deviation: beta_max = float32(beta * image_max(whole image)),
    not the window's own maximum (the device would need a reduction and a host wait per batch for that)."""
    S = int(S)
    c = np.shape(images[0])[2] if len(images) else 0
    out_img = np.empty((len(records), c, S, S), np.float32)
    out_mask = np.empty((len(records), 1, S, S), np.float32)
    for i, rec in enumerate(records):
        p = rec["params"]
        img, mask = window(images[rec["img"]], masks[rec["img"]], rec["y0"], rec["x0"], S)
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
