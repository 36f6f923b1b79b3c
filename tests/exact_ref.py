"""Exact-integer references, fixtures and guard buffers for the convolution routes (CPU only: importable without a GPU).

Why exact: with integer data, |x|, |w| small and K * max|a| * max|b| < 2^24 for the K products summed into one output,
every fp32 partial sum is an exact integer in ANY summation order.  The MFMA paths (bf16 products are exact in fp32;
fp32 MFMA is exact fp32) and the CPU reference then produce the same number, and the expected bf16 output is the
round-to-nearest-even of that number (csrc/common.h from_f32) -- the check is equality per element.

Layout of the references: NHWC tensors [N, H, W, C] (the kernels' activation layout), weights in PyTorch layout
(Conv2d [Cout][Cin][3][3], ConvTranspose2d [Cin][Cout][2][2]).  Accumulation is fp64, or fp32 where the exactness rule
holds (asserted before use: fp32 GEMMs are then exact and several times faster).  The references run on the device of
their inputs: on integer data fp64 arithmetic has no rounding at all (every value and partial sum is far below 2^53), so
the result is the same exact integer on the host or on a GPU, whatever library or summation order computes it."""
import math
import os
import re

import torch
import torch.nn.functional as F

EXACT_LIMIT = 1 << 24
SENTINEL = 2.0 ** 60                     # finite input fill outside a view: s * SENTINEL + t stays finite for |s| <= 4
NAN_BITS = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5}     # distinctive quiet-NaN pattern of output guards
INT_VIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
ONEHOT_VALUES = (1, 2, -1)


# ---------------------------------------------------------------------------------------------------- exactness rule
def assert_exact(k, amax, bmax):
    """k products of magnitude <= amax * bmax summed into one output: every partial sum must stay below 2^24."""
    amax, bmax = float(amax), float(bmax)
    assert k * amax * bmax < EXACT_LIMIT, f"not exact in fp32: K={k} * {amax} * {bmax} >= 2^24"


def value_range(k, bmax=None):
    """Largest r in (2, 1) such that k products of an operand in {-r..r} with one bounded by bmax (default: the same r)
    stay exact."""
    for r in (2, 1):
        if k * r * (r if bmax is None else bmax) < EXACT_LIMIT:
            return r
    raise AssertionError(f"K={k}: no exact integer range")


def _acc(k, a, b, fast):
    if fast:
        assert_exact(k, a.abs().max(), b.abs().max())
        return torch.float32
    return torch.float64


# ---------------------------------------------------------------------------------------------------- storage rounding
def round_bf16(x):
    """fp32 -> bf16 round-to-nearest-even by bit arithmetic (what from_f32 / v_cvt_pk_bf16_f32 do); NaN stays NaN."""
    x = x.to(torch.float32).contiguous()
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    r = torch.where(torch.isnan(x), (b >> 16) | 0x40, r) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16).view(torch.bfloat16)


def to_storage(x, dtype):
    """Exact value (fp64 / fp32 tensor) -> what a kernel storing through `dtype` writes."""
    x = x.to(torch.float32)
    return round_bf16(x) if dtype == torch.bfloat16 else x


# ---------------------------------------------------------------------------------------------------- references
def _chunks(n, pix, cap=1 << 22):
    step = max(1, cap // max(pix, 1))
    for i in range(0, n, step):
        yield i, min(n, i + step)


def conv3x3_fwd(x, w, d, bias=None, fast=False):
    """Dilated 3x3 convolution, padding = dilation: x [N,H,W,Ci], w [Co,Ci,3,3] -> [N,H,W,Co]; one GEMM per tap."""
    n, h, wd, ci = x.shape
    co = w.shape[0]
    dt = _acc(9 * ci, x, w, fast)
    out = torch.empty(n, h, wd, co, dtype=dt, device=x.device)
    w = w.to(device=x.device, dtype=dt)
    for i0, i1 in _chunks(n, h * wd * max(ci, co)):
        xp = F.pad(x[i0:i1].to(dt), (0, 0, d, d, d, d))
        acc = torch.zeros((i1 - i0) * h * wd, co, dtype=dt, device=x.device)
        for ky in range(3):
            for kx in range(3):
                acc += xp[:, ky * d:ky * d + h, kx * d:kx * d + wd, :].reshape(-1, ci) @ w[:, :, ky, kx].t()
        out[i0:i1] = acc.view(i1 - i0, h, wd, co)
    if bias is not None:
        out += bias.to(out)
    return out


def conv3x3_dgrad(dy, w, d, fast=False):
    """Input gradient of conv3x3_fwd: dx[y,x,ci] = sum dy[y-(ky-1)d, x-(kx-1)d, co] w[co,ci,ky,kx]."""
    n, h, wd, co = dy.shape
    ci = w.shape[1]
    dt = _acc(9 * co, dy, w, fast)
    out = torch.empty(n, h, wd, ci, dtype=dt, device=dy.device)
    w = w.to(device=dy.device, dtype=dt)
    for i0, i1 in _chunks(n, h * wd * max(ci, co)):
        dp = F.pad(dy[i0:i1].to(dt), (0, 0, d, d, d, d))
        acc = torch.zeros((i1 - i0) * h * wd, ci, dtype=dt, device=dy.device)
        for ky in range(3):
            for kx in range(3):
                acc += dp[:, (2 - ky) * d:(2 - ky) * d + h, (2 - kx) * d:(2 - kx) * d + wd, :].reshape(-1, co) @ w[:, :, ky, kx]
        out[i0:i1] = acc.view(i1 - i0, h, wd, ci)
    return out


def conv3x3_wgrad(x, dy, d, fast=False):
    """Weight gradient of conv3x3_fwd: dw[co,ci,ky,kx] = sum over pixels dy[p,co] * x_shifted(ky,kx)[p,ci]."""
    n, h, wd, ci = x.shape
    co = dy.shape[-1]
    dt = _acc(n * h * wd, x, dy, fast)
    dw = torch.zeros(co, ci, 3, 3, dtype=dt, device=x.device)
    for i0, i1 in _chunks(n, h * wd * max(ci, co)):
        xp = F.pad(x[i0:i1].to(dt), (0, 0, d, d, d, d))
        g = dy[i0:i1].to(dt).reshape(-1, co).t()
        for ky in range(3):
            for kx in range(3):
                dw[:, :, ky, kx] += g @ xp[:, ky * d:ky * d + h, kx * d:kx * d + wd, :].reshape(-1, ci)
    return dw


def conv3x3_fwd_onehot(x, route, co, d):
    """conv3x3_fwd for a one-hot routed weight (onehot_conv3x3): output channel c = v * input channel ci shifted by its
    tap -- a gather, no GEMM (exact in fp32 for integer inputs of any size)."""
    n, h, wd, _ = x.shape
    ci_of, tap_of, v_of = (r.to(x.device) for r in route)
    xp = F.pad(x.to(torch.float32), (0, 0, d, d, d, d))
    out = torch.empty(n, h, wd, co, dtype=torch.float32, device=x.device)
    for t in range(9):
        cs = (tap_of == t).nonzero().flatten()
        if cs.numel():
            ky, kx = divmod(t, 3)
            out[..., cs] = xp[:, ky * d:ky * d + h, kx * d:kx * d + wd, :][..., ci_of[cs]] * v_of[cs].float()
    return out


def conv3x3_dgrad_onehot(dy, route, ci, d):
    """conv3x3_dgrad for a one-hot routed weight: dx[ci] = sum over the output channels routed from ci of v * dy shifted."""
    n, h, wd, _ = dy.shape
    ci_of, tap_of, v_of = (r.to(dy.device) for r in route)
    dp = F.pad(dy.to(torch.float32), (0, 0, d, d, d, d))
    out = torch.zeros(n, h, wd, ci, dtype=torch.float32, device=dy.device)
    for t in range(9):
        cs = (tap_of == t).nonzero().flatten()
        if cs.numel():
            ky, kx = divmod(t, 3)
            out.index_add_(3, ci_of[cs], dp[:, (2 - ky) * d:(2 - ky) * d + h, (2 - kx) * d:(2 - kx) * d + wd, :][..., cs]
                           * v_of[cs].float())
    return out


def conv3x3_wgrad_separable(a, u, dy, d):
    """conv3x3_wgrad for a separable input x[p, ci] = a[p] * u[ci] (a [N,H,W]): dw[co,ci,t] = u[ci] * sum_p a_t[p] dy[p,co]
    -- nine matrix-vector products instead of nine GEMMs."""
    n, h, wd = a.shape
    co = dy.shape[-1]
    assert_exact(n * h * wd, float(a.abs().max()) * float(u.abs().max()), dy.abs().max())
    ap = F.pad(a.to(torch.float64), (d, d, d, d))
    g = dy.to(torch.float64).reshape(-1, co)
    s = torch.empty(co, 3, 3, dtype=torch.float64, device=dy.device)
    for ky in range(3):
        for kx in range(3):
            s[:, ky, kx] = ap[:, ky * d:ky * d + h, kx * d:kx * d + wd].reshape(-1) @ g
    return s[:, None] * u.to(s)[None, :, None, None]


def convT2x2_fwd(x, w, bias=None, fast=False):
    """ConvTranspose2d(k=2, s=2): x [N,h,w,Ci], w [Ci,Co,2,2] -> [N,2h,2w,Co]."""
    n, h, wd, ci = x.shape
    co = w.shape[1]
    dt = _acc(ci, x, w, fast)
    out = torch.empty(n, 2 * h, 2 * wd, co, dtype=dt, device=x.device)
    xm = x.to(dt).reshape(-1, ci)
    w = w.to(device=x.device, dtype=dt)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2, :] = (xm @ w[:, :, a, b]).view(n, h, wd, co)
    if bias is not None:
        out += bias.to(out)
    return out


def convT2x2_dgrad(dup, w, fast=False):
    n, h2, w2, co = dup.shape
    ci = w.shape[0]
    dt = _acc(4 * co, dup, w, fast)
    acc = torch.zeros(n * (h2 // 2) * (w2 // 2), ci, dtype=dt, device=dup.device)
    w = w.to(device=dup.device, dtype=dt)
    for a in range(2):
        for b in range(2):
            acc += dup[:, a::2, b::2, :].to(dt).reshape(-1, co) @ w[:, :, a, b].t()
    return acc.view(n, h2 // 2, w2 // 2, ci)


def convT2x2_wgrad(x, dup, fast=False):
    n, h, wd, ci = x.shape
    co = dup.shape[-1]
    dt = _acc(n * h * wd, x, dup, fast)
    xm = x.to(dt).reshape(-1, ci).t()
    dw = torch.empty(ci, co, 2, 2, dtype=dt, device=x.device)
    for a in range(2):
        for b in range(2):
            dw[:, :, a, b] = xm @ dup[:, a::2, b::2, :].to(dt).reshape(-1, co)
    return dw


def first_fwd(x_nchw, w, d, bias=None, fast=False):
    """First-layer convolution (C_in 1 or 3, NCHW input) -> NHWC output."""
    return conv3x3_fwd(x_nchw.permute(0, 2, 3, 1), w, d, bias, fast)


def first_wgrad(x_nchw, dy, d, fast=False):
    return conv3x3_wgrad(x_nchw.permute(0, 2, 3, 1), dy, d, fast)


def first_dgrad(dy, w, d, fast=False):
    """Input gradient of the first layer, NCHW."""
    return conv3x3_dgrad(dy, w, d, fast).permute(0, 3, 1, 2)


def bn_relu(y, scale, shift):
    """relu(scale * y + shift) per channel (last dim), fp64."""
    return torch.relu(y.to(torch.float64) * scale.to(y.device, torch.float64) + shift.to(y.device, torch.float64))


def maxpool2(a):
    n, h, w, c = a.shape
    return a.reshape(n, h // 2, 2, w // 2, 2, c).amax(dim=(2, 4))


def colsum(x):
    """Per-channel column sums of an NHWC (or [pixels, C]) tensor, fp64."""
    return x.to(torch.float64).reshape(-1, x.shape[-1]).sum(0)


# ---------------------------------------------------------------------------------------------------- BatchNorm, head, loss
# Plain fp64 statements of the arithmetic around the convolutions.  Inputs are the values as STORED (what the kernel reads);
# every result is the exact mathematical value in fp64.  Where a fixture makes the fp32 arithmetic exact, the kernel's fp32
# result equals the fp32 rounding of these values; elsewhere a test compares against them under a bound (within_bound).
EPS32 = 2.0 ** -24                       # unit roundoff of fp32
EPS64 = 2.0 ** -53                       # unit roundoff of fp64


def _f64(t, dev):
    return None if t is None else t.to(device=dev, dtype=torch.float64)


def bn_finalize(parts, count, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """nn.BatchNorm2d training statistics from [rows, 2, C] partial (sum, sum of squares) rows: batch mean, biased variance,
    rstd = 1 / sqrt(var + eps), scale = gamma * rstd, shift = beta - mean * scale, and the running buffers updated with
    momentum and the UNBIASED variance (var * count / (count - 1))."""
    dev = parts.device
    p = parts.to(torch.float64)
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + float(eps))
    scale = _f64(gamma, dev) * rstd
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=_f64(beta, dev) - mean * scale)
    if running_mean is not None:
        m = float(momentum)
        unbiased = var * (count / (count - 1.0 if count > 1 else 1.0))
        out["running_mean"] = (1.0 - m) * _f64(running_mean, dev) + m * mean
        out["running_var"] = (1.0 - m) * _f64(running_var, dev) + m * unbiased
    return out


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, conv_bias=None):
    """Eval-mode BatchNorm folded with the conv bias: scale = gamma / sqrt(rv + eps), shift = beta + (bias - rm) * scale."""
    dev = gamma.device
    scale = _f64(gamma, dev) / torch.sqrt(_f64(running_var, dev) + float(eps))
    bias = torch.zeros_like(scale) if conv_bias is None else _f64(conv_bias, dev)
    return dict(scale=scale, shift=_f64(beta, dev) + (bias - _f64(running_mean, dev)) * scale)


def bn_frozen_affine(gamma, beta, running_mean, running_var, eps):
    """Frozen statistics: mean = rm, rstd = 1 / sqrt(rv + eps), scale = gamma * rstd, shift = beta - rm * scale."""
    dev = gamma.device
    rstd = 1.0 / torch.sqrt(_f64(running_var, dev) + float(eps))
    scale = _f64(gamma, dev) * rstd
    mean = _f64(running_mean, dev)
    return dict(mean=mean, rstd=rstd, scale=scale, shift=_f64(beta, dev) - mean * scale)


def pool_argmax(a):
    """Index k = 2 * row + col of the FIRST maximum of every 2x2 window of a [N, H, W, C] (ATen's max_pool2d tie rule)."""
    n, h, w, c = a.shape
    win = a.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)
    hit = (win == win.amax(dim=3, keepdim=True)).to(torch.uint8)
    return hit.argmax(dim=3)             # first True: torch.argmax returns the first maximal index


def pool_scatter(dpool, arg, h, w):
    """The pooled gradient routed to the window arg-max: [N, H/2, W/2, C] -> [N, H, W, C]."""
    n, hq, wq, c = dpool.shape
    g = torch.zeros(n, hq, wq, 4, c, dtype=torch.float64, device=dpool.device)
    g.scatter_(3, arg.unsqueeze(3), dpool.to(torch.float64).unsqueeze(3))
    return g.reshape(n, hq, wq, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)


def bn_relu_bwd(y, scale, shift, mean, rstd, gamma, dskip=None, dpool=None, dtype=torch.float32, frozen=False, sums=None):
    """Backward of y -> BatchNorm -> ReLU (-> skip and/or 2x2 max-pool).  y, dskip: [N, H, W, C]; dpool [N, H/2, W/2, C].
    The pool arg-max is taken on the activation as stored (relu(scale y + shift) rounded through `dtype`), first maximum
    wins.  gh = [scale y + shift > 0] * gradient, xhat = (y - mean) rstd; S1 = sum gh, S2 = sum gh xhat, S3 = sum xhat.
    k1 = gamma rstd, k2 = k1 S1 / M, k3 = k1 S2 / M; dy = k1 gh - k2 - k3 xhat; dgamma = S2, dbeta = S1, dbias = -k3 S3.
    frozen: k2 = k3 = 0, dbias = k1 S1.  sums: (S1, S2, S3) given by a producer (the pre_parts forms) instead."""
    dev = y.device
    n, h, w, c = y.shape
    yd = y.to(torch.float64)
    sc, sh, mu, rs, ga = (_f64(t, dev) for t in (scale, shift, mean, rstd, gamma))
    nrm = yd * sc + sh
    gin = torch.zeros_like(yd) if dskip is None else dskip.to(torch.float64).clone()
    if dpool is not None:
        a = to_storage(torch.relu(nrm), dtype).to(torch.float64)
        gin += pool_scatter(dpool, pool_argmax(a), h, w)
    gh = torch.where(nrm > 0, gin, torch.zeros_like(gin))
    xh = (yd - mu) * rs
    if sums is None:
        sums = tuple(t.reshape(-1, c).sum(0) for t in (gh, gh * xh, xh))
    s1, s2, s3 = (_f64(t, dev) for t in sums)
    m = float(n * h * w)
    k1 = ga * rs
    if frozen:
        k2, k3, dbias = torch.zeros_like(k1), torch.zeros_like(k1), k1 * s1
    else:
        k2, k3 = k1 * s1 / m, k1 * s2 / m
        dbias = -k3 * s3
    dy = k1 * gh - k2 - k3 * xh
    # dy = fmaf(k1, gh, -k2) - k3 * xh in fp32 from the fp32 k1, k2, k3 (gh and xh are exact in the fixtures): the stored k2
    # and k3 are roundings of the exact ones (E each; none at a power-of-two count), k3 * xh rounds (E), the fused term
    # rounds once (E (|k1 gh| + |k2|)), the difference once more (E of everything): at most
    # E (2 |k1 gh| + 3 |k2| + 4 |k3 xh|) to first order, within the 4 E (...) below at any pixel count.
    dy_bound = 4 * EPS32 * ((k1 * gh).abs() + k2.abs() + (k3 * xh).abs())
    out = dict(dy=dy, dy_bound=dy_bound, gh=gh, xh=xh, s1=s1, s2=s2, s3=s3, dgamma=s2, dbeta=s1, dbias=dbias, k1=k1, k2=k2, k3=k3)
    out.update(bn_bwd_coeff_bounds(k2, k3, dbias))
    return out


def bn_bwd_coeff_bounds(k2, k3, dbias):
    """How far the DOUBLE value that bn_bwd_finalize_kernel rounds to fp32 can lie from the fp64 reference when the pixel
    count M is not a power of two (at a power of two, with the integer fixtures, every operation is exact and the tests ask
    for equality).  The kernel forms a = gamma rstd (exact in double: two 24-bit significands), then a S / M in double -- one
    product and one division, each within 2^-53 -- and rounds to fp32 once; the reference does the same two operations in
    fp64, in whatever association, with the same two roundings at most: the two doubles differ by at most 4 * 2^-53 |k|.
    dbias = -(a S2 / M) S3 has one more product on each side: 6 * 2^-53 |dbias|.  exact_ref.within_bound then accepts the fp32
    rounding of the reference, and its neighbour only where the reference lies that close to an fp32 rounding boundary.
    (Far tighter than one fp32 division and one fp32 product, 2 * 2^-24 |k|, which an fp32 finalize would need.)"""
    return dict(k2_bound=4 * EPS64 * k2.abs(), k3_bound=4 * EPS64 * k3.abs(), dbias_bound=6 * EPS64 * dbias.abs())


def head_dz(dprobs, probs):
    """Gradient of the head's pre-sigmoid output: dz = dprobs * p * (1 - p)."""
    p = probs.to(torch.float64)
    return dprobs.to(torch.float64) * p * (1.0 - p)


def head_fwd(a, w, b, n, h, wd):
    """Conv2d(C, OC, 1) + sigmoid: a [P, C] NHWC pixels -> z, probs [N, OC, H, W]."""
    z = a.to(torch.float64) @ _f64(w, a.device).t() + _f64(b, a.device)
    z = z.view(n, h, wd, -1).permute(0, 3, 1, 2)
    return z, torch.sigmoid(z)


def head_bwd(dprobs, probs, a, w, dtype=torch.float32, bn=None):
    """Backward of head_fwd: dz [P, OC], dW [OC, C] = sum dz a, db [OC] = sum dz, da [P, C] = dz @ W.  bn = (y, scale, shift,
    mean, rstd) of the stage whose activation `a` is: its BatchNorm-backward sums taken on da as stored (rounded through
    `dtype`), as unetdc_head_bwd_bnstats leaves them."""
    dev = a.device
    oc = w.shape[0]
    dz = head_dz(dprobs, probs).permute(0, 2, 3, 1).reshape(-1, oc)
    ad = a.to(torch.float64)
    wd = _f64(w, dev)
    out = dict(dz=dz, dw=dz.t() @ ad, db=dz.sum(0), da=dz @ wd)
    if bn is not None:
        y, sc, sh, mu, rs = bn
        yd = y.to(torch.float64)
        g = to_storage(out["da"], dtype).to(torch.float64)
        gh = torch.where(yd * _f64(sc, dev) + _f64(sh, dev) > 0, g, torch.zeros_like(g))
        xh = (yd - _f64(mu, dev)) * _f64(rs, dev)
        out.update(gh=gh, xh=xh, s1=gh.sum(0), s2=(gh * xh).sum(0), s3=xh.sum(0))
    return out


def _log_clamped(x):
    """torch's BCE clamp: max(log x, -100) (log 0 = -inf -> -100)."""
    return torch.log(x).clamp_min(-100.0)


def focal_dice(p, t, alpha, gamma, ratio, smooth):
    """The fused Focal + Dice loss of csrc/loss.hip on [nimg, hw] maps, fp64: bce = -(t max(log p, -100) + (1-t) max(log(1-p),
    -100)), pt = exp(-bce), focal = mean alpha (1-pt)^gamma bce; dice_i = (2 I + s) / (P + T + s);
    loss = ratio focal + (1 - ratio)(1 - mean dice).  d loss / d p for grad_out = 1: the clamped log contributes no
    gradient (its derivative term is dropped where log <= -100), dice through c1 = 2 / U, c2 = (2 I + s) / U^2."""
    p, t = p.to(torch.float64), t.to(torch.float64)
    nimg, hw = p.shape
    numel = float(nimg * hw)
    lp, lq = torch.log(p), torch.log1p(-p)
    bce = -(t * lp.clamp_min(-100.0) + (1 - t) * lq.clamp_min(-100.0))
    pt = torch.exp(-bce)
    om = 1 - pt
    focal = alpha * om.pow(gamma) * bce
    dbce = -(torch.where(lp > -100, t / p, torch.zeros_like(p)) - torch.where(lq > -100, (1 - t) / (1 - p), torch.zeros_like(p)))
    dfocal = alpha * (gamma * om.pow(gamma - 1) * pt * bce + om.pow(gamma)) * dbce
    inter, psum, tsum = (p * t).sum(1), p.sum(1), t.sum(1)
    u = psum + tsum + smooth
    dice = (2 * inter + smooth) / u
    c1, c2 = 2 / u, (2 * inter + smooth) / (u * u)
    loss = ratio * focal.sum() / numel + (1 - ratio) * (1 - dice.mean())
    dp = ratio * dfocal / numel - (1 - ratio) / nimg * (t * c1[:, None] - c2[:, None])
    return dict(loss=loss, dp=dp, focal=focal, dfocal=dfocal, bce=bce, c1=c1, c2=c2, inter=inter, psum=psum, tsum=tsum)


_TINY = 2.0 ** -147                      # absolute slack of one fp32 operation whose result is subnormal


def _widen(lo, hi, rel):
    """[lo, hi] widened by `rel` times the larger magnitude (plus the subnormal slack): one rounded fp32 operation."""
    m = torch.maximum(lo.abs(), hi.abs()) * rel + _TINY
    return lo - m, hi + m


def _mul(alo, ahi, blo, bhi):
    c = torch.stack([alo * blo, alo * bhi, ahi * blo, ahi * bhi])
    return c.amin(0), c.amax(0)


def focal_dice_bounds(p, t, alpha, gamma, ratio, smooth, grad_out, nsum):
    """Interval bounds on what csrc/loss.hip's fp32 arithmetic can produce: every fp32 operation is widened by one rounding
    (2^-24 relative), logf / log1pf / expf / powf by 4 ulp, and the three fp32 sums per map by nsum roundings (nsum = the
    longest chain of additions any partial sum goes through).  alpha / gamma / ratio / smooth must be the fp32 values the
    kernel receives.  Returns (loss_lo, loss_hi) and per-element (dp_lo, dp_hi) for dprobs = grad_out * d loss / d p."""
    E, LIB = EPS32, 8 * EPS32
    p, t = p.to(torch.float64), t.to(torch.float64)
    nimg, hw = p.shape
    numel = float(nimg * hw)
    lp, lq = torch.log(p), torch.log1p(-p)
    tl, ql = (t * lp.clamp_min(-100.0)).abs(), ((1 - t) * lq.clamp_min(-100.0)).abs()
    bce = tl + ql
    db = 2 * LIB * (tl + ql) + _TINY
    b_lo, b_hi = (bce - db).clamp_min(0.0), bce + db
    pt_lo, pt_hi = torch.exp(-b_hi) * (1 - LIB) - _TINY, (torch.exp(-b_lo) * (1 + LIB) + _TINY).clamp_max(1.0)
    pt_lo = pt_lo.clamp_min(0.0)
    om_lo, om_hi = ((1 - pt_hi) * (1 - E) - _TINY).clamp_min(0.0), (1 - pt_lo) * (1 + E) + _TINY
    if gamma == 2.0:
        o1_lo, o1_hi = om_lo, om_hi
    else:
        o1_lo, o1_hi = om_lo.pow(gamma - 1) * (1 - LIB) - _TINY, om_hi.pow(gamma - 1) * (1 + LIB) + _TINY
        o1_lo = o1_lo.clamp_min(0.0)
    og_lo, og_hi = (o1_lo * om_lo * (1 - E) - _TINY).clamp_min(0.0), o1_hi * om_hi * (1 + E) + _TINY
    f_lo, f_hi = alpha * og_lo * b_lo * (1 - 2 * E) - _TINY, alpha * og_hi * b_hi * (1 + 2 * E) + _TINY
    # forward: the sums of focal terms, p * t, p and t
    ferr = nsum * E * f_hi.abs().sum()
    F_lo, F_hi = f_lo.sum() - ferr, f_hi.sum() + ferr
    pt_, ps_, ts_ = p * t, p, t
    I, P, T = pt_.sum(1), ps_.sum(1), ts_.sum(1)
    dI, dP, dT = (nsum * E * x.abs().sum(1) for x in (pt_, ps_, ts_))
    U_lo, U_hi = (P - dP) + (T - dT) + smooth, (P + dP) + (T + dT) + smooth
    I_lo, I_hi = I - dI, I + dI
    D_lo, D_hi = ((2 * I_lo + smooth) / U_hi).sum(), ((2 * I_hi + smooth) / U_lo).sum()
    loss_lo = ratio * F_lo / numel + (1 - ratio) * (1 - D_hi / nimg)
    loss_hi = ratio * F_hi / numel + (1 - ratio) * (1 - D_lo / nimg)
    loss_lo, loss_hi = _widen(loss_lo, loss_hi, 2 * E)
    # backward
    a1 = torch.where(lp > -100, t / p, torch.zeros_like(p)).abs()
    a2 = torch.where(lq > -100, (1 - t) / (1 - p), torch.zeros_like(p)).abs()
    dbce = -(torch.where(lp > -100, t / p, torch.zeros_like(p)) - torch.where(lq > -100, (1 - t) / (1 - p), torch.zeros_like(p)))
    dd = 3 * E * a1 + 5 * E * a2 + _TINY
    d_lo, d_hi = dbce - dd, dbce + dd
    A_lo = ((gamma * o1_lo * pt_lo * b_lo) * (1 - 3 * E) + og_lo) * (1 - E)
    A_hi = ((gamma * o1_hi * pt_hi * b_hi) * (1 + 3 * E) + og_hi) * (1 + E) + _TINY
    df_lo, df_hi = _widen(*_mul(alpha * A_lo, alpha * A_hi, d_lo, d_hi), 2 * E)
    c1_lo, c1_hi = 2 / U_hi * (1 - E), 2 / U_lo * (1 + E)
    c2_lo, c2_hi = (2 * I_lo + smooth) / (U_hi * U_hi) * (1 - E), (2 * I_hi + smooth) / (U_lo * U_lo) * (1 + E)
    kf = torch.tensor(ratio / numel, dtype=torch.float64).float().double().item()
    kd = (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(ratio, dtype=torch.float32)) / torch.tensor(float(nimg))
    kd = float(kd.double())
    u_lo, u_hi = _widen(kf * df_lo, kf * df_hi, E)
    tc_lo, tc_hi = _widen(*_mul(t, t, c1_lo[:, None], c1_hi[:, None]), E)
    v_lo, v_hi = _widen(tc_lo - c2_hi[:, None], tc_hi - c2_lo[:, None], E)
    w_lo, w_hi = _widen(kd * v_lo, kd * v_hi, E)
    r_lo, r_hi = _widen(u_lo - w_hi, u_hi - w_lo, E)
    g = float(grad_out)
    dp_lo, dp_hi = _widen(*_mul(torch.full_like(r_lo, g), torch.full_like(r_hi, g), r_lo, r_hi), E)
    return (loss_lo, loss_hi), (dp_lo, dp_hi)


def within_bound(got, ref, bound, dtype):
    """Elementwise check of a stored value against an fp64 reference whose fp32 computation can be off by `bound`: the stored
    value must lie in [store(ref - bound), store(ref + bound)] where store is the storage rounding (round-to-nearest-even is
    monotone, so this is 'the rounding of the reference, or either neighbour when the reference lies within the bound of a
    rounding boundary'; bound 0 = equality).  NaN-strict.  Returns a boolean mask of the elements that fail."""
    ref, bound = ref.to(torch.float64), torch.as_tensor(bound, dtype=torch.float64, device=ref.device)
    lo = to_storage(ref - bound, dtype).to(torch.float64)
    hi = to_storage(ref + bound, dtype).to(torch.float64)
    g = got.to(device=ref.device, dtype=torch.float64).reshape(ref.shape)
    return ~((g >= lo) & (g <= hi))


def sum_is_exact(terms, res):
    """Every fp32 partial sum of `terms` ([rows, C], multiples of `res`) is exact in any order: sum |terms| / res < 2^24."""
    t = terms.to(torch.float64).reshape(-1, terms.shape[-1]) / res
    return bool((t == t.round()).all()) and float(t.abs().sum(0).max()) < EXACT_LIMIT


# ---------------------------------------------------------------------------------------------------- optimizer
_FLUSH = 2.0 ** -126                     # absolute slack of one fp32 operation whose result is subnormal, flushed or not


def adam_step(p, m, v, g, step, lr, beta1, beta2, eps, grad_scale=1.0):
    """One Adam step in fp64 from the state as it was just before it (csrc/optim.hip, torch's _fused_adam_ formulation):
    g <- grad_scale g;  m <- m + (1 - b1)(g - m);  v <- b2 v + (1 - b2) g^2;
    p <- p - lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).   Returns (p, m, v), fp64."""
    p, m, v, g = (t.to(torch.float64) for t in (p, m, v, g))
    g = g * grad_scale
    m = m + (1 - beta1) * (g - m)
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return p - lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


def adam_bounds(p, m, v, g, step, lr, beta1, beta2, eps, grad_scale=1.0):
    """Per-element bounds on how far the fp32 arithmetic of csrc/optim.hip adam_update can lie from adam_step: (bp, bm, bv).

    Interval arithmetic over the kernel's operation sequence; the inputs p, m, v, g are exact (the fp32 values it reads).
      constants  gscale, omb1 = 1-b1, b2, omb2 = 1-b2, eps, step_size = lr/bc1, inv_bc2_sqrt = 1/sqrt(bc2): formed in
                 double, rounded to fp32 once -> each one in c (1 +- E)            (E = 2^-24; double errors are < 2^-50)
      g' = g * gscale                  one rounding (none when grad_scale == 1: the product is exact)
      m' = fmaf(omb1, g' - m, m)       g' - m rounded, then ONE rounding of the fused result
      v' = fmaf(v, b2, omb2 g' g')     (omb2 g') g' two roundings, then ONE rounding of the fused result; v' >= 0
      s  = sqrtf(v')                   correctly rounded by default for HIP; 2E allowed
      den = s * inv_bc2_sqrt + eps     two roundings (whether or not the compiler contracts it to one fma)
      q  = m' / den                    2E allowed, as for sqrtf; den > 0 for eps > 0
      p' = p - step_size * q           two roundings (contracted or not)
    Every rounded result r also carries an absolute 2^-126 (a subnormal result, flushed to zero or not).  The interval of each
    result is widened by the rounding of its larger end; the bound is the distance from the exact fp64 value (adam_step with
    the exact hyper-parameters) to the farther end.  First-order in E, so a few ulp of each output: a wrong bias correction,
    a lost grad_scale or a lost update is off by far more.  Returns fp64 tensors."""
    E = EPS32
    p, m, v, g = (t.to(torch.float64) for t in (p, m, v, g))

    def wid(lo, hi, rel=E):
        s = torch.maximum(lo.abs(), hi.abs()) * rel + _FLUSH
        return lo - s, hi + s

    def const(c):
        c = torch.tensor(float(c), dtype=torch.float64, device=p.device)
        return c * (1 - E), c * (1 + E)

    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    if grad_scale == 1.0:
        g_lo, g_hi = g, g
    else:
        g_lo, g_hi = wid(*_mul(g, g, *const(grad_scale)))
    d_lo, d_hi = wid(g_lo - m, g_hi - m)
    o_lo, o_hi = _mul(*const(1 - beta1), d_lo, d_hi)
    m_lo, m_hi = wid(o_lo + m, o_hi + m)
    t_lo, t_hi = wid(*_mul(*const(1 - beta2), g_lo, g_hi))
    t_lo, t_hi = wid(*_mul(t_lo, t_hi, g_lo, g_hi))
    b_lo, b_hi = _mul(v, v, *const(beta2))
    v_lo, v_hi = wid(b_lo + t_lo.clamp_min(0.0), b_hi + t_hi)
    v_lo = v_lo.clamp_min(0.0)
    s_lo, s_hi = wid(v_lo.sqrt(), v_hi.sqrt(), 2 * E)
    s_lo = s_lo.clamp_min(0.0)
    e_lo, e_hi = const(eps)
    den_lo, den_hi = wid(*_mul(s_lo, s_hi, *const(1 / math.sqrt(bc2))))
    den_lo, den_hi = wid(den_lo + e_lo, den_hi + e_hi)
    assert bool((den_lo > 0).all()), "adam_bounds: the denominator may reach 0 (eps = 0 and v = 0)"
    q_lo, q_hi = wid(*_mul(m_lo, m_hi, 1 / den_hi, 1 / den_lo), 2 * E)
    u_lo, u_hi = wid(*_mul(*const(lr / bc1), q_lo, q_hi))
    np_lo, np_hi = wid(p - u_hi, p - u_lo)
    rp, rm, rv = adam_step(p, m, v, g, step, lr, beta1, beta2, eps, grad_scale)
    far = lambda lo, hi, r: torch.maximum(r - lo, hi - r)        # noqa: E731
    return far(np_lo, np_hi, rp), far(m_lo, m_hi, rm), far(v_lo, v_hi, rv)


def pack_conv3x3(w):
    """Host form of the packed 3x3 images (engine.PackedWeights): w [Co,Ci,3,3] -> (w_fwd [9][Co][Ci], w_dgrad [9][Ci][Co]) with
    tap t = 3 ky + kx; the dgrad image holds the flipped taps, w_dgrad[t] = w[..., 8 - t]^T."""
    co, ci = w.shape[:2]
    t = w.reshape(co, ci, 9)
    return t.permute(2, 0, 1).contiguous(), t.flip(2).permute(2, 1, 0).contiguous()


def pack_convT2x2(w):
    """Host form of the packed ConvTranspose2d images: w [Ci,Co,2,2] -> (w_fwd [4][Co][Ci] (= [4*Co][Ci]), w_dgrad [4][Ci][Co])
    with ab = 2 a + b the output sub-pixel."""
    ci, co = w.shape[:2]
    t = w.reshape(ci, co, 4)
    return t.permute(2, 1, 0).contiguous(), t.permute(2, 0, 1).contiguous()


def conv3x3_packed(x, wk, d):
    """x [N,H,W,C] through one packed 3x3 image wk [9][Cout][C] as nine shifted GEMMs (the packed operand as the kernels read
    it, K = C contiguous): forward with w_fwd, input gradient with w_dgrad (the flipped taps make it the same form)."""
    n, h, wd, c = x.shape
    xp = F.pad(x, (0, 0, d, d, d, d))
    acc = torch.zeros(n * h * wd, wk.shape[1], dtype=x.dtype)
    for t in range(9):
        ky, kx = divmod(t, 3)
        acc += xp[:, ky * d:ky * d + h, kx * d:kx * d + wd, :].reshape(-1, c) @ wk[t].t()
    return acc.view(n, h, wd, -1)


def convT2x2_packed(x, wk):
    """x [N,H,W,C] through one packed 2x2 image wk [4][Cout][C]: out[2y + a, 2x + b] = x[y, x] @ wk[2a + b]^T for the forward
    image (w_fwd); for the dgrad image it is the adjoint, dx[y, x] = sum_ab dup[2y + a, 2x + b] @ wk[ab]^T (convT2x2_packed_adj)."""
    n, h, wd, c = x.shape
    out = torch.empty(n, 2 * h, 2 * wd, wk.shape[1], dtype=x.dtype)
    for ab in range(4):
        a, b = divmod(ab, 2)
        out[:, a::2, b::2, :] = (x.reshape(-1, c) @ wk[ab].t()).view(n, h, wd, -1)
    return out


def convT2x2_packed_adj(dup, wk):
    n, h2, w2, c = dup.shape
    acc = torch.zeros(n * (h2 // 2) * (w2 // 2), wk.shape[1], dtype=dup.dtype)
    for ab in range(4):
        a, b = divmod(ab, 2)
        acc += dup[:, a::2, b::2, :].reshape(-1, c) @ wk[ab].t()
    return acc.view(n, h2 // 2, w2 // 2, -1)


# ---------------------------------------------------------------------------------------------------- fixtures
def ints(shape, r, g, lo=None, device="cpu"):
    """Uniform integers in {lo..r} (lo = -r by default) as fp32."""
    lo = -r if lo is None else lo
    return torch.randint(lo, r + 1, tuple(shape), generator=g, device=device).to(torch.float32)


def dense_conv3x3(co, ci, g, r=2):
    """Dense integer weight; asymmetric (no tap-flip or transpose symmetry a row/column or tap-order swap could hide in)."""
    w = ints((co, ci, 3, 3), r, g)
    w[:, :, 0, 0] += (w[:, :, 0, 0] == w[:, :, 2, 2]).float() * (1 - 2 * (w[:, :, 0, 0] > 0).float())
    return w


def onehot_route(co, ci):
    """Output channel c reads input channel (5c + 3) % ci at tap c % 9 with weight (1, 2, -1)[(c // 9) % 3]: both the
    input channel and the tap vary with c, so every tap and every 64/128-channel block of the input appears."""
    c = torch.arange(co)
    return (5 * c + 3) % ci, c % 9, torch.tensor(ONEHOT_VALUES)[(c // 9) % 3]


def onehot_conv3x3(co, ci):
    ci_of, tap_of, v_of = onehot_route(co, ci)
    w = torch.zeros(co, ci, 9)
    w[torch.arange(co), ci_of, tap_of] = v_of.float()
    return w.view(co, ci, 3, 3), (ci_of, tap_of, v_of)


def onehot_convT2x2(ci, co):
    """Every (co, tap) of the transposed convolution reads one input channel: (5co + 3t + 1) % ci, weight (1, 2, -1)."""
    w = torch.zeros(ci, co, 4)
    for t in range(4):
        c = torch.arange(co)
        w[(5 * c + 3 * t + 1) % ci, c, t] = torch.tensor(ONEHOT_VALUES)[(c + t) % 3].float()
    return w.view(ci, co, 2, 2)


def pow2(c, g, exps=(0, 1)):
    """Per-channel powers of two (BatchNorm scales that keep s * x exact)."""
    e = torch.tensor(exps)[torch.randint(0, len(exps), (c,), generator=g)]
    return torch.pow(2.0, e.float())


def describe_mismatch(got, exp, what, route=None):
    """First differing element of two NHWC tensors as (n, y, x, c) [and the one-hot (ci, tap) of c]."""
    got, exp = got.to(torch.float64), exp.to(torch.float64)
    bad = (got != exp) & ~(torch.isnan(got) & torch.isnan(exp))
    nb = int(bad.sum())
    if nb == 0:
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    msg = f"{what}: {nb} of {bad.numel()} elements differ; first at {idx}: got {float(got[idx])} expected {float(exp[idx])}"
    if route is not None and len(idx) == 4:
        c = idx[3]
        msg += f" (co {c} reads ci {int(route[0][c])} at tap {int(route[1][c])})"
    return msg


# ---------------------------------------------------------------------------------------------------- guard buffers
class Carved:
    """A [rows, cols] view at column `off` of a [rows, ld] region that sits `margin` rows into a larger flat buffer."""

    def __init__(self, buf, rows, cols, ld, off, margin):
        self.buf, self.rows, self.cols, self.ld, self.off, self.margin = buf, rows, cols, ld, off, margin
        self.view = buf[margin * ld:(margin + rows) * ld].view(rows, ld)[:, off:off + cols]


def carve(rows, cols, ld, off, dtype, margin, fill="nan", device="cuda"):
    """Output views (fill='nan') are surrounded by the NaN pattern of NAN_BITS; input views (fill='sentinel') by SENTINEL;
    fill=None leaves the buffer as allocated (the caller writes the view)."""
    assert 0 <= off and off + cols <= ld
    buf = torch.empty((rows + 2 * margin) * ld, dtype=dtype, device=device)
    if fill == "nan":
        buf.view(INT_VIEW[dtype]).fill_(_signed(NAN_BITS[dtype], dtype))
    elif fill == "sentinel":
        buf.fill_(SENTINEL)
    return Carved(buf, rows, cols, ld, off, margin)


def _signed(bits, dtype):
    width = 16 if dtype == torch.bfloat16 else 32
    return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def guard_violations(c):
    """Positions (row relative to the view, column) outside the view whose bits differ from the NaN pattern."""
    pat = _signed(NAN_BITS[c.buf.dtype], c.buf.dtype)
    bits = c.buf.view(INT_VIEW[c.buf.dtype]).clone()
    bits[c.margin * c.ld:(c.margin + c.rows) * c.ld].view(c.rows, c.ld)[:, c.off:c.off + c.cols] = pat
    bad = (bits != pat).nonzero().flatten()
    return [(int(i) // c.ld - c.margin, int(i) % c.ld) for i in bad[:8].cpu()], int(bad.numel())


def assert_guard(c, what):
    where, nbad = guard_violations(c)
    assert nbad == 0, f"{what}: {nbad} element(s) written outside the view (rows {c.rows}, cols [{c.off}, {c.off + c.cols}) " \
                      f"of ld {c.ld}); first (row, col): {where}"


def stats_guard(declared, dtype=torch.float32, extra=256, device="cuda"):
    """A stats / parts buffer of the size the header declares, followed by `extra` guard elements."""
    return carve(1, declared, declared + extra, 0, dtype, 0, device=device)


# ---------------------------------------------------------------------------------------------------- argument table
# The C-ABI parameter names of every replayed symbol, in order (include/unetdc_hip.h; tests/test_exact_ref_cpu.py parses
# the header and fails if a name or position moves).  Shapes, leading dimensions, dtype, pointers and workspaces are
# recognised by name below, with the ctypes argument kinds of unet_dc_segmentation_amd._lib.SIGNATURES.
ARGS = {
    "unetdc_conv3x3_fwd": "x ldx w_fwd bias scale shift y ldy stats_part stats_rows n h w cin cout dilation dtype s",
    "unetdc_conv3x3_fwd_bnin": "x_raw ldx in_scale in_shift w_fwd bias y ldy stats_part stats_rows act_out ldact n h w cin cout "
                               "dilation dtype s",
    "unetdc_conv3x3_wgrad_bnin": "x_raw ldx in_scale in_shift dy lddy dw workspace workspace_bytes n h w cin cout dilation dtype s",
    "unetdc_conv3x3_dgrad": "dy lddy w_dgrad dx lddx n h w cin cout dilation dtype s",
    "unetdc_conv3x3_wgrad": "x ldx dy lddy dw workspace workspace_bytes n h w cin cout dilation dtype s",
    "unetdc_conv3x3_first_fwd": "x_nchw w bias scale shift y ldy stats_part n h wd cin cout dilation dtype s",
    "unetdc_conv3x3_first_wgrad": "x_nchw dy lddy dw workspace workspace_bytes n h w cin cout dilation dtype s",
    "unetdc_conv3x3_first_dgrad": "dy lddy w dx_nchw n h wd cin cout dilation dtype s",
    "unetdc_conv3x3_first_wgrad_bn": "x_nchw dz lddz y ldy scale shift mean rstd coeffs dw workspace workspace_bytes n h w cin cout "
                                     "dilation dtype s",
    "unetdc_convT2x2_fwd": "x ldx w_fwd bias up ldup n h w cin cout dtype s",
    "unetdc_convT2x2_dgrad": "dup lddup w_dgrad dx lddx n h w cin cout dtype s",
    "unetdc_convT2x2_wgrad": "x ldx dup lddup dw workspace workspace_bytes n h w cin cout dtype s",
    "unetdc_bn_relu_apply": "y ldy scale shift a lda pooled ldp n h w c dtype s",
    "unetdc_conv3x3_dgrad_bnstats": "dy lddy w_dgrad dx lddx y_prev ldy_prev scale shift mean rstd parts parts_floats nparts n h w "
                                    "cin cout dilation dtype s",
    "unetdc_convT2x2_dgrad_bnstats": "dup lddup w_dgrad dx lddx y_prev ldy_prev scale shift mean rstd parts parts_floats nparts n h "
                                     "w cin cout dtype s",
    "unetdc_conv3x3_dgrad_colsum": "dy lddy w_dgrad dx lddx colsum c0 c workspace workspace_bytes n h w cin cout dilation dtype s",
    "unetdc_bn_finalize": "stats_part rows count gamma beta eps momentum running_mean running_var scale shift mean rstd c s",
    "unetdc_bn_eval_affine": "gamma beta running_mean running_var conv_bias eps scale shift c s",
    "unetdc_bn_frozen_affine": "gamma beta running_mean running_var eps scale shift mean rstd c s",
    "unetdc_bn_relu_bwd": "dskip ldskip dpool ldpool y ldy scale shift mean rstd gamma dy lddy dgamma dbeta dbias workspace "
                          "workspace_bytes pre_parts pre_nparts n h w c dtype s",
    "unetdc_bn_relu_bwd_frozen": "dskip ldskip dpool ldpool y ldy scale shift mean rstd gamma dy lddy dgamma dbeta dbias workspace "
                                 "workspace_bytes pre_parts pre_nparts n h w c dtype s",
    "unetdc_bn_relu_bwd_head": "dprobs probs head_w y ldy scale shift mean rstd gamma dy lddy dgamma dbeta dbias workspace "
                               "workspace_bytes pre_parts pre_nparts n h w c dtype s",
    "unetdc_bn_relu_bwd_coeffs": "pre_parts pre_nparts gamma rstd dgamma dbeta dbias coeffs n h w c s",
    "unetdc_head_fwd": "a lda w b probs n h wd c oc dtype s",
    "unetdc_head_fwd_bn": "y ldy scale shift w b probs n h wd c oc dtype s",
    "unetdc_head_bwd": "dprobs probs a lda w da ldda dw db workspace workspace_bytes n h wd c oc dtype s",
    "unetdc_head_bwd_bnstats": "dprobs probs a lda w da ldda dw db workspace workspace_bytes y_prev ldy_prev scale shift mean rstd "
                               "parts parts_floats nparts n h wd c oc dtype s",
    "unetdc_focal_dice_loss_fwd": "probs target loss_out coef workspace workspace_bytes nimg hw alpha gamma ratio smooth s",
    "unetdc_focal_dice_loss_bwd": "probs target coef grad_out dprobs nimg hw alpha gamma ratio s",
}
ARGS = {k: tuple(v.split()) for k, v in ARGS.items()}
SHAPE_NAMES = ("n", "h", "w", "wd", "cin", "cout", "dilation", "c0", "c", "oc", "rows", "count", "pre_nparts", "nimg", "hw",
               "parts_floats")
# the fields of every replayed symbol a runner needs (tests/test_exact_ref_cpu.py checks them against the table)
REPLAY_KEYS = {"unetdc_bn_finalize": ("rows", "count", "c", "eps", "momentum", "ptr:running_mean"),
               "unetdc_bn_eval_affine": ("c", "eps", "ptr:conv_bias"),
               "unetdc_bn_frozen_affine": ("c", "eps"),
               "unetdc_bn_relu_bwd_coeffs": ("n", "h", "w", "c", "pre_nparts"),
               "unetdc_focal_dice_loss_fwd": ("nimg", "hw", "alpha", "gamma", "ratio", "smooth", "workspace_bytes"),
               "unetdc_focal_dice_loss_bwd": ("nimg", "hw", "alpha", "gamma", "ratio")}
FLOAT_NAMES = ("eps", "momentum", "alpha", "gamma", "ratio", "smooth")
CANON = {"wd": "w"}                      # the first-layer symbols call the image width `wd` (their `w` is the weight)


def arg_kinds(argtypes):
    """ctypes argument types -> 'P' (pointer), 'I' (int), 'F' (float / double), 'L' (int64)."""
    return ["P" if t.__name__ == "c_void_p" else "I" if t.__name__ == "c_int" else "F" if t.__name__ in ("c_float", "c_double")
            else "L" for t in argtypes]


def positions(sym, kinds):
    """name -> position for the arguments of `sym` that the replay reads: shapes (int / int64), lds, dtype, scalar parameters
    (float), pointers, workspace."""
    out = {}
    for i, (name, kind) in enumerate(zip(ARGS[sym], kinds)):
        if kind in "IL" and (name in SHAPE_NAMES or name.startswith("ld") or name == "dtype"):
            out[CANON.get(name, name)] = i
        elif kind == "F" and name in FLOAT_NAMES:
            out[name] = i
        elif kind == "P" and name != "s":
            out["ptr:" + name] = i
        elif name == "workspace_bytes":
            out[name] = i
    return out


def parse_header(path=None):
    """{function name: (parameter names...)} of include/unetdc_hip.h."""
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unetdc_hip.h")
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t|const char\*)\s+(unetdc_\w+)\s*\(([^)]*)\)\s*;", src):
        params = [p.strip() for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        out[m.group(1)] = tuple(re.findall(r"(\w+)\s*$", p)[0] for p in params)
    return out
