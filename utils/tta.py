"""Test-time augmentation over the dihedral group D4: the network runs on flipped and rotated copies of
its input, every output is mapped back, and the outputs are averaged.

Everything here is the ONE derivation of the rule: ``expand_numpy`` / ``mean_numpy`` are the host path of
``unetdc_dihedral_expand_f32`` / ``unetdc_dihedral_mean_f32`` (csrc/tta.hip: same values, same order of the fp32 operations),
``mean_numpy64`` is the fp64 yardstick of the tests.  Only numpy is needed, torch for ``predict_tta_cpu``.

Variant v in 0..7 of a square plane: hflip = v & 4, k = v & 3, ``np.rot90(plane[:, ::-1] if hflip else plane, k)`` -- the flip
first, then k counter-clockwise quarter turns, the order of the training augmentation (utils/data_loader.py:TrainAugment).
"""
import numpy as np

TTA_SIZES = (1, 2, 4, 8)
_LISTS = {1: (0,), 2: (0, 4), 4: (0, 4, 2, 6), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
MIN_SIDE, MAX_SIDE, MAX_IMAGES, MAX_CHANNELS = 16, 4096, 4096, 4          # the kernels' limits


def check_tta(N):
    """N: the number of variants per image, one of TTA_SIZES."""
    if isinstance(N, bool) or int(N) != N or int(N) not in TTA_SIZES:
        raise ValueError(f"{N} variants: one of {', '.join(map(str, TTA_SIZES))}")
    return int(N)


def variants(N):
    """The ordered variant list of N: identity; + hflip; the flip group (identity, hflip, rot180, vflip); all of D4."""
    return _LISTS[check_tta(N)]


def variant(plane, v):
    """Variant v of [..., S, S]: the flip, then the rotation."""
    return np.rot90(plane[..., ::-1] if v & 4 else plane, v & 3, axes=(-2, -1))


def variant_inverse(plane, v):
    """The inverse of ``variant``: the rotation back, then the flip."""
    r = np.rot90(plane, -(v & 3), axes=(-2, -1))
    return r[..., ::-1] if v & 4 else r


def _square(a, ndim, what):
    a = np.asarray(a)
    if a.ndim != ndim or a.shape[-1] != a.shape[-2] or a.shape[-1] % 16 or not MIN_SIDE <= a.shape[-1] <= MAX_SIDE:
        raise ValueError(f"{what}: square planes with a side that is a multiple of 16 in {MIN_SIDE}..{MAX_SIDE}, not {a.shape}")
    return a


def expand_numpy(x, N):
    """x: [n, C, S, S] -> [n * N, C, S, S]: item b * N + i is variant variants(N)[i] of image b (a permutation: bit-exact)."""
    x, vs = _square(x, 4, "expand"), variants(N)
    out = np.empty((x.shape[0] * len(vs),) + x.shape[1:], x.dtype)
    for i, v in enumerate(vs):
        out[i::len(vs)] = variant(x, v)
    return out


def _mean(p, N, dtype):
    p, vs = _square(p, 3, "mean"), variants(N)
    if p.shape[0] % len(vs):
        raise ValueError(f"mean: {p.shape[0]} items are no multiple of {len(vs)} variants")
    acc = variant_inverse(p[0::len(vs)], vs[0]).astype(dtype)
    for i, v in enumerate(vs[1:], 1):
        acc = acc + variant_inverse(p[i::len(vs)], v).astype(dtype)       # list order, every add rounded in `dtype`
    return acc / dtype(len(vs))


def mean_numpy(p, N):
    """p: fp32 [n * N, S, S], item b * N + i the output on variant i of image b -> fp32 [n, S, S]: every item mapped back through
    the inverse of its variant, summed in list order in fp32 (acc = q_0, acc = acc + q_i), one division by float(N)."""
    return _mean(np.asarray(p, np.float32), N, np.float32)


def mean_env_numpy(p, N):
    """p as for mean_numpy -> (mean, lo, hi), fp32 [n, S, S] each: mean_numpy bit for bit, and the per-pixel minimum and maximum
    over the mapped-back items (np.minimum / np.maximum: the envelope of unetdc_dihedral_mean_env_f32).  Only lo <= hi holds: the
    rounded fp32 mean of equal values may miss them, so nothing may assume lo <= mean <= hi."""
    p, vs = _square(np.asarray(p, np.float32), 3, "mean"), variants(N)
    mean = mean_numpy(p, N)
    lo = hi = variant_inverse(p[0::len(vs)], vs[0])
    for i, v in enumerate(vs[1:], 1):
        q = variant_inverse(p[i::len(vs)], v)
        lo, hi = np.minimum(lo, q), np.maximum(hi, q)
    return mean, np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def mean_numpy64(p, N):
    """The same rule in fp64 (the yardstick of the tests)."""
    return _mean(p, N, np.float64)


def groups(n, N, batch):
    """The chunk rule of both paths: the n images go in groups of G = max(1, batch // N); a group of g images is expanded once,
    its g * N items are forwarded in slices of `batch`, and one mean follows.  -> [(b0, g)]."""
    G = max(1, max(1, int(batch)) // N)
    return [(b0, min(G, n - b0)) for b0 in range(0, n, G)]


def predict_tta_cpu(model, x, N, batch, envelope=False):
    """CPU path of unet_dc_segmentation_amd.tta.predict_tta: x [n, C, S, S] fp32 (torch, on the CPU) -> [n, 1, S, S] fp32
    probabilities: expand_numpy of every group, its items through `model` in slices of `batch` under no_grad, mean_numpy.
    envelope: -> (mean, lo, hi) of mean_env_numpy instead, three tensors of that shape."""
    import torch
    N, batch = check_tta(N), max(1, int(batch))
    xn = _square(x.detach().numpy(), 4, "predict_tta_cpu")
    out = np.empty((3 if envelope else 1, xn.shape[0], 1) + xn.shape[2:], np.float32)
    with torch.no_grad():
        for b0, g in groups(xn.shape[0], N, batch):
            items = torch.from_numpy(expand_numpy(xn[b0:b0 + g], N))
            p = torch.cat([model(items[i:i + batch])[:, 0].float() for i in range(0, g * N, batch)])
            if envelope:
                out[:, b0:b0 + g, 0] = mean_env_numpy(p.numpy(), N)
            else:
                out[0, b0:b0 + g, 0] = mean_numpy(p.numpy(), N)
    return tuple(torch.from_numpy(o) for o in out) if envelope else torch.from_numpy(out[0])
