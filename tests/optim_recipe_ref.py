"""References and bounds of the optimizer recipe (csrc/optim.hip: unetdc_grad_norm, unetdc_adam_step_ex),
next to tests/exact_ref.py's adam_step / adam_bounds, which they build on."""
import math

import numpy as np
import torch

from tests import exact_ref as X

E = X.EPS32                                   # 2^-24: the relative error of one fp32 rounding
# numpy mirrors of unetdc_adam_desc and unetdc_step_ctl (include/unetdc_hip.h)
DESC = np.dtype([("p", "<u8"), ("m", "<u8"), ("v", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("g_off", "<i8"), ("begin", "<i8"),
                 ("numel", "<i8"), ("a", "<i4"), ("b", "<i4"), ("kind", "<i4"), ("flags", "<i4")])
CTL = np.dtype([("sumsq", "<f8"), ("norm", "<f8"), ("gscale_eff", "<f4"), ("skip", "<i4"), ("steps", "<i8"), ("clipped", "<i8"),
                ("skipped", "<i8"), ("norm_sum", "<f8")])
assert DESC.itemsize == 80 and CTL.itemsize == 56
# the first stage of unetdc_grad_norm: elements a workgroup covers per trip, and the cap on the number of partials (all of
# which the one-workgroup finaliser reads itself; past NORM_PARTS * NORM_BLOCK elements the workgroups take several trips)
NORM_BLOCK, NORM_PARTS = 4096, 2048


def sumsq_ref(g, grad_scale=1.0):
    """grad_scale^2 * sum g^2 of the fp32 values, in fp64 (torch's pairwise sum: its own error is far below the bound)."""
    return float((g.to(torch.float64) ** 2).sum()) * grad_scale * grad_scale


def sumsq_rel_bound(n):
    """Relative bound on the device's sumsq against the exact sum: (n + 2) 2^-53.

    The kernel's operation sequence: every term (double)g * (double)g is EXACT (a 24-bit significand squared has 48 bits, the
    exponent range of fp64 covers every fp32 square), so the only errors are the fp64 additions.  All terms are >= 0, hence
    every partial sum is at most the total S and each of the n - 1 additions -- in whatever fixed order the threads, the shuffle
    trees and the finaliser take them -- errs by at most 2^-53 S (1 + O(n 2^-53)): (n - 1) 2^-53 S to first order.  The
    finaliser then multiplies by grad_scale twice, two more roundings: (n + 1) 2^-53.  The last 2^-53 covers the second-order
    terms (n^2 2^-106 < 2^-53 for n < 2^26, the sizes the tests use).  The reference's own error (sumsq_ref: torch's pairwise
    fp64 sum, about log2(n) 2^-53) fits in what the first-order term leaves unused: no thread, shuffle tree or finaliser chain of
    the kernel is anywhere near n - 1 additions long."""
    return (n + 2) * 2.0 ** -53


def ctl_expect(norm, grad_scale, max_norm):
    """(coef, gscale_eff) the record must hold for the DEVICE's own norm: clip_grad_norm_'s coefficient in double, the product
    with grad_scale formed in double and rounded to fp32 once."""
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    return coef, np.float32(grad_scale * coef)


def step_ref(p, m, v, g, step, lr, b1, b2, eps, gscale, factor=None, decayed=None):
    """fp64 reference and per-element bounds of one unetdc_adam_step_ex update at the gradient scale `gscale` (the device's
    gscale_eff).  factor = 1 - lr * weight_decay in double (None: nothing is decayed), decayed = a bool mask of the elements of
    flagged tensors (None: all): the kernel multiplies p by the fp32 rounding of the factor and rounds the product, before
    adam_update -- against the exact factor that is one rounding of the constant and one of the product, 2 * 2^-24 |p factor|
    on top of adam_bounds (evaluated at the decayed p).  Unflagged elements get adam_bounds alone.
    Returns ((p, m, v) reference, (bp, bm, bv))."""
    p64 = p.to(torch.float64)
    extra = 0.0
    if factor is not None:
        dec = p64 * factor
        add = 2 * E * dec.abs() + 2.0 ** -126
        if decayed is None:
            p64, extra = dec, add
        else:
            p64, extra = torch.where(decayed, dec, p64), torch.where(decayed, add, torch.zeros_like(add))
    ref = X.adam_step(p64, m, v, g, step, lr, b1, b2, eps, gscale)
    bp, bm, bv = X.adam_bounds(p64, m, v, g, step, lr, b1, b2, eps, gscale)
    return ref, (bp + extra, bm, bv)


def ema_ref(e0, p1, ema_decay):
    """e0 + (1 - d)(p1 - e0) in fp64 from the device's p1, with 1 - d the fp32 constant the launcher forms (double, rounded
    once), and the bound of the kernel's two roundings: p1 - e0 (scaled by 1 - d), then the fused multiply-add."""
    omd = float(np.float32(1.0 - ema_decay))
    e0, p1 = e0.to(torch.float64), p1.to(torch.float64)
    diff = p1 - e0
    ref = e0 + omd * diff
    return ref, E * (omd * diff.abs() + ref.abs()) * (1 + 4 * E) + 2 * 2.0 ** -126


def ema_decay_at(decay, step):
    return min(float(decay), (1.0 + step) / (10.0 + step))


def cosine_lr(step, base, lr_min, total, warmup):
    """The closed form of utils/lr_schedule.py's cosine schedule."""
    if step < warmup:
        scale = (step + 1) / warmup
    else:
        scale = 1.0
    q = min(max((step - warmup) / (total - warmup), 0.0), 1.0)
    return (lr_min + (base - lr_min) * 0.5 * (1.0 + math.cos(math.pi * q))) * scale
