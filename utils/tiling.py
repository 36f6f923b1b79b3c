"""Tiled inference at native resolution: the tile plan, the reflect-101 fold, the blend weights and the
numpy restatement of the two device kernels (csrc/tile.hip).

An image of h x w pixels is cut into overlapping T x T tiles, the network runs on the tiles, and the tile probabilities are
blended back into one h x w map.  Everything here is the ONE derivation of the rules: ``gather_numpy`` / ``blend_numpy`` are
the host path of ``unetdc_tile_gather_u8_to_chw_f32`` / ``unetdc_tile_blend_f32`` (same values, same order of the fp32
operations), ``blend_numpy64`` is the fp64 yardstick of the tests.  Only numpy is needed, torch for ``predict_tiled_cpu``.
"""
import numpy as np

MIN_TILE, MAX_TILE = 32, 4096          # the plan's limits; the kernels themselves take any multiple of 16 up to TILE_MAX_T
MAX_SIDE = 16384                       # image sides, as everywhere on the image side


def check_tile(T, O):
    """The limits of both paths: T a multiple of 16 (the network's rule) in 32..4096, 0 <= O <= T / 2."""
    T, O = int(T), int(O)
    if T % 16 or not MIN_TILE <= T <= MAX_TILE:
        raise ValueError(f"tile size {T}: a multiple of 16 in {MIN_TILE}..{MAX_TILE}")
    if not 0 <= 2 * O <= T:
        raise ValueError(f"tile overlap {O}: 0..{T // 2} (at most half the tile size {T})")
    return T, O


def axis_origins(dim, T, O):
    """Origins of the tiles along one axis of length dim: one tile at 0 when dim <= T, else the least number n of tiles that
    cover the axis with an overlap of at least O, n = ceil((dim - O) / (T - O)), spread evenly: o_k = k (dim - T) // (n - 1).
    The first origin is 0, the last dim - T; no tile leaves the image."""
    dim = int(dim)
    if dim < 1:
        raise ValueError(f"axis length {dim}")
    if dim <= T:
        return [0]
    n = -((O - dim) // (T - O))
    return [(k * (dim - T)) // (n - 1) for k in range(n)]


def tile_plan(h, w, T, O):
    """(yo, xo): the per-axis origin lists.  Tile number t = ty * len(xo) + tx has its corner at (yo[ty], xo[tx])."""
    T, O = check_tile(T, O)
    return axis_origins(h, T, O), axis_origins(w, T, O)


def fold(i, dim):
    """Reflect-101 (numpy.pad's "reflect") of any integer coordinate(s) into 0..dim-1, with as many reflections as needed:
    period 2 (dim - 1); dim == 1 maps everything to 0."""
    i = np.asarray(i, dtype=np.int64)
    if dim == 1:
        return np.zeros_like(i)
    p = 2 * (dim - 1)
    m = np.mod(i, p)
    return np.where(m < dim, m, p - m)


def axis_weights(T, O):
    """int64 [T]: w(i) = min(i + 1, T - i, max(O, 1)): a ramp of O steps at either end of a tile, flat between."""
    i = np.arange(T, dtype=np.int64)
    return np.minimum(np.minimum(i + 1, T - i), max(int(O), 1))


def gather_numpy(img, T, O):
    """img: uint8 [H, W, C] -> fp32 [n_tiles, C, T, T]: tile t holds float(v) / 255.0f of the pixels at its corner and on,
    coordinates outside the image folded back (an image smaller than the tile)."""
    return gather_at_numpy(img, T, *tile_plan(np.shape(img)[0], np.shape(img)[1], T, O))


def gather_at_numpy(img, T, yo, xo):
    """gather_numpy at given origin lists: what unetdc_tile_gather_u8_to_chw_f32 computes for ANY origins and tile size."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("gather_numpy needs an [H, W, C] uint8 array")
    h, w = img.shape[:2]
    r = np.arange(T)
    out = np.empty((len(yo) * len(xo), img.shape[2], T, T), np.float32)
    for ty, y0 in enumerate(yo):
        rows = img[fold(y0 + r, h)]
        for tx, x0 in enumerate(xo):
            out[ty * len(xo) + tx] = rows[:, fold(x0 + r, w)].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return out


def _blend(tiles, h, w, T, O, dtype):
    T, O = check_tile(T, O)
    yo, xo = tile_plan(h, w, T, O)
    tiles = np.asarray(tiles)
    if tiles.shape != (len(yo) * len(xo), T, T):
        raise ValueError(f"blend: {tiles.shape} tiles, the plan of {h} x {w} has {(len(yo) * len(xo), T, T)}")
    wt = axis_weights(T, O)
    num, den = np.zeros((h, w), dtype), np.zeros((h, w), dtype)
    for ty, y0 in enumerate(yo):                              # tile order: every pixel sums its tiles in ascending (ty, tx)
        hh = min(T, h - y0)
        for tx, x0 in enumerate(xo):
            ww = min(T, w - x0)
            wgt = (wt[:hh, None] * wt[None, :ww]).astype(dtype)                # an integer, exact in either type
            num[y0:y0 + hh, x0:x0 + ww] += wgt * tiles[ty * len(xo) + tx, :hh, :ww].astype(dtype)    # product rounded, then the sum
            den[y0:y0 + hh, x0:x0 + ww] += wgt
    return num / den


def blend_numpy(tiles, h, w, T, O):
    """tiles: fp32 [n_tiles, T, T] probabilities of the plan of (h, w, T, O) -> fp32 [h, w]: sum(wy wx p) / sum(wy wx) over
    the tiles that cover a pixel, both sums in fp32 in tile order (product and sum rounded separately), one division."""
    return _blend(np.asarray(tiles, np.float32), h, w, T, O, np.float32)


def blend_numpy64(tiles, h, w, T, O):
    """The same rule in fp64 (the yardstick of the tests)."""
    return _blend(tiles, h, w, T, O, np.float64)


def predict_tiled_cpu(model, img_u8, T, O, batch, tta=1, envelope=False):
    """CPU path of unet_dc_segmentation_amd.tiling.predict_tiled: img_u8 [H, W, C] uint8 (numpy) -> fp32 [H, W] probabilities
    (numpy): the tiles of gather_numpy through `model` in chunks of `batch` under no_grad, then blend_numpy.  tta > 1: every
    tile's probabilities are the mean over its `tta` flipped and rotated variants (utils.tta.predict_tta_cpu, `batch` items per
    forward) before the blend.  envelope: -> (mean, lo, hi), three maps: lo and hi are the blend of the per-tile envelopes
    (utils.tta.mean_env_numpy per tile, each through the same blend_numpy)."""
    import torch
    img_u8 = np.asarray(img_u8)
    tiles = torch.from_numpy(gather_numpy(img_u8, T, O))
    batch = max(1, int(batch))
    if envelope:
        from utils.tta import predict_tta_cpu
        return tuple(blend_numpy(p[:, 0].numpy(), img_u8.shape[0], img_u8.shape[1], T, O)
                     for p in predict_tta_cpu(model, tiles, tta, batch, envelope=True))
    if tta != 1:
        from utils.tta import predict_tta_cpu
        probs = predict_tta_cpu(model, tiles, tta, batch)[:, 0]
    else:
        with torch.no_grad():
            probs = torch.cat([model(tiles[i:i + batch])[:, 0] for i in range(0, len(tiles), batch)])
    return blend_numpy(probs.numpy(), img_u8.shape[0], img_u8.shape[1], T, O)
