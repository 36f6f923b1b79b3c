"""Exact and fp64-bounded tests of the kernels around the convolutions: BatchNorm statistics, the BatchNorm + ReLU (+ max-pool)
backward in all its forms, the eval and frozen affines, the sigmoid head and the fused Focal + Dice loss.

Comparison rule (tests/exact_ref.py has the references):
  - where a fixture makes the fp32 arithmetic exact (integer / power-of-two / dyadic values, every fp32 partial sum below
    2^24 -- asserted on the fixture), the stored value must EQUAL the storage rounding of the fp64 reference, at ANY pixel
    count: BatchNorm statistics (eps = 0: the totals are multiples of the count), BatchNorm-backward sums, dgamma / dbeta,
    k1, the frozen forms' dbias, the head's dW / db / dA and its BatchNorm sums; at a power-of-two pixel count also k2, k3
    and dbias;
  - k2 = k1 S1 / M, k3 = k1 S2 / M and dbias = -k3 S3 at a pixel count M that is not a power of two: the fp32 rounding of the
    fp64 reference, or its neighbour only where the reference lies within a few 2^-53 of an fp32 rounding boundary
    (exact_ref.bn_bwd_coeff_bounds: the kernel divides in double and rounds once);
  - everything else (dy = fmaf(k1, gh, -k2) - k3 xhat, sigmoid, logs and powers of the loss, running statistics) is compared
    element by element with the fp64 reference under a bound derived from the fp32 operations of that output
    (exact_ref.within_bound: in bf16, either neighbour only where the reference lies within the bound of a rounding boundary).
Every output starts as NaN inside guards; workspaces and partial-row buffers are guarded from the size the header declares
(including the 64 spare rows after pre_nparts); every check is NaN-strict.  The runners take the header's argument names, so
tests/test_gpu_exact.py replays them at the shapes a training step issues."""
import ctypes
import math

import pytest
import torch

from tests import exact_ref as X

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd._lib import call

TD = {0: torch.float32, 1: torch.bfloat16}
DTYPES = {"f32": 0, "bf16": 1}
MARGIN = 3
E = X.EPS32


def conv_helpers():
    from tests import test_gpu_exact                # put / out buffers of the convolution runners (imported late: it imports us)
    return test_gpu_exact


def lib():
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dgen(g):
    return torch.Generator(device="cuda").manual_seed(int(torch.randint(1 << 30, (1,), generator=g)))


def dints(shape, r, g, lo=None):
    """Integer fixture drawn on the device (seeded from g)."""
    return X.ints(shape, r, dgen(g), lo, device="cuda")


def vec(t):
    """A per-channel fp32 input on the device."""
    return t.to(torch.float32).contiguous().cuda()


def outv(n):
    """A guarded fp32 output vector of n elements (NaN inside and around)."""
    return X.carve(1, n, n, 0, torch.float32, 64)


def inout(t):
    """An fp32 in/out vector (running statistics) inside NaN guards."""
    c = X.carve(1, t.numel(), t.numel(), 0, torch.float32, 64)
    c.view.copy_(t.reshape(1, -1).cuda())
    return c


def check(got, ref, bound, dtype, what, shape=None):
    """got (a Carved output or a tensor) against the fp64 reference under `bound` (0 = equality after storage rounding)."""
    view = got.view if isinstance(got, X.Carved) else got
    bad = X.within_bound(view.reshape(ref.shape), ref, bound, dtype)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        g = float(view.reshape(ref.shape)[idx])
        b = float(torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)[idx]) if torch.is_tensor(bound) else float(bound)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at {idx}"
                             f"{' of ' + str(shape) if shape else ''}: got {g!r}, reference {float(ref[idx])!r} +- {b:g}")
    if isinstance(got, X.Carved):
        X.assert_guard(got, what)


def pow2_count(m):
    return m > 0 and m & (m - 1) == 0


# ---------------------------------------------------------------------------------------------------- BatchNorm statistics
def finalize_parts(rows, count, c, g, dev="cuda"):
    """[rows, 2, C] integer partial rows whose totals give mean m in {-2..2} and variance 4^k (k in {0, 1, 2}) per channel:
    with eps = 0 every statistic is exact AT ANY COUNT (the totals are the integers m count and (var + m^2) count, and a
    correctly rounded double division gives m and var + m^2 back: tests/test_exact_ref_cpu.py).  Rows carry a zero-sum integer
    wobble, so no row equals another.  Where rows is the number of 256-pixel blocks of a count that is not a multiple of 256,
    the rows are weighted as a producer leaves them: the last one carries the count % 256 remaining pixels' share."""
    m = X.ints((c,), 2, g).double()
    var = torch.pow(4.0, torch.randint(0, 3, (c,), generator=g).double())
    tot = torch.stack([m * count, (var + m * m) * count]).to(torch.int64)          # [2, C]
    i = torch.arange(rows).view(rows, 1, 1)
    noise = torch.randint(-3, 4, (rows, 2, c), generator=g)
    if rows > 1 and rows == -(-count // 256) and count % 256:
        wts = torch.full((rows,), 256, dtype=torch.int64)
        wts[-1] = count % 256
        share = (tot.view(1, 2, c) * wts.view(rows, 1, 1)) // count                # floor toward -inf: |share| <= |tot|
        share[0] += tot - share.sum(0)
        if rows > 2:                               # (row 0 also takes the rounding remainder, so compare with a middle row)
            assert int(share[-1].abs().max()) < int(share[1].abs().max()), "the last row should carry the smaller share"
    else:
        base, rem = tot // rows, tot % rows
        share = base.view(1, 2, c) + (i < rem.view(1, 2, c)).to(torch.int64)
    parts = share + noise - noise.roll(1, 0)
    assert torch.equal(parts.sum(0), tot)
    assert int(parts.abs().max()) < X.EXACT_LIMIT
    if rows > 512:                              # the fp32 pre-reduction adds groups of ceil(rows / 64) rows
        rpg = (rows + 63) // 64
        grp = parts.abs()[: (rows // rpg) * rpg].view(-1, rpg, 2, c).sum(1)
        assert int(grp.max()) + rpg * int(parts.abs().max()) < X.EXACT_LIMIT
    return parts.to(torch.float32).to(dev), m, var


def bn_finalize(kw, seed=31):
    rows, count, c = kw["rows"], kw["count"], kw["c"]
    eps, mom = kw.get("eps", 0.0), kw.get("momentum", 0.1)
    running = kw.get("ptr:running_mean", True)
    g = gen(seed)
    parts, _, _ = finalize_parts(rows, count, c, g)
    gamma = X.pow2(c, g, (-1, 0, 1)) * (1 - 2 * (torch.rand(c, generator=g) < 0.3).float())
    beta = X.ints((c,), 3, g)
    rm0, rv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    st = X.stats_guard((rows + 64) * 2 * c)                      # the header's contract: rows + 64 rows
    st.view.view(-1)[: rows * 2 * c] = parts.reshape(-1)
    outs = {k: outv(c) for k in ("scale", "shift", "mean", "rstd")}
    rm, rv = (inout(rm0), inout(rv0)) if running else (None, None)
    gd, bd = vec(gamma), vec(beta)
    call("unetdc_bn_finalize", st.view.data_ptr(), rows, count, gd.data_ptr(), bd.data_ptr(), float(eps), float(mom),
         None if rm is None else rm.view.data_ptr(), None if rv is None else rv.view.data_ptr(),
         *(outs[k].view.data_ptr() for k in ("scale", "shift", "mean", "rstd")), c, stream())
    torch.cuda.synchronize()
    eps32, mom32 = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(mom, dtype=torch.float32))
    ref = X.bn_finalize(parts.double(), count, gamma, beta, eps32, mom32, rm0, rv0)
    what = f"bn_finalize(rows {rows}, count {count}, C {c}, eps {eps32:g})"
    exact = eps32 == 0.0
    check(outs["mean"], ref["mean"], 0, torch.float32, what + " mean")
    check(outs["rstd"], ref["rstd"], 0 if exact else 2.0 ** -40 * ref["rstd"], torch.float32, what + " rstd")
    check(outs["scale"], ref["scale"], 0 if exact else 2 * E * ref["scale"].abs(), torch.float32, what + " scale")
    sb = 0 if exact else 2 * E * (ref["shift"].abs() + 2 * (ref["mean"] * ref["scale"]).abs())
    check(outs["shift"], ref["shift"], sb, torch.float32, what + " shift")
    X.assert_guard(st, what + " partial rows")
    if running:                                   # (1 - m) * r + m * x in fp32, x rounded to fp32 once: 4 roundings
        for k, r0, x in (("running_mean", rm0, ref["mean"]), ("running_var", rv0, ref["var"] * count / max(count - 1, 1))):
            b = 4 * E * ((1 - mom32) * r0.double().cuda().abs() + mom32 * x.abs()) + 2.0 ** -140
            check(rm if k == "running_mean" else rv, ref[k], b, torch.float32, f"{what} {k}")
    return None


def bn_affine(kw, frozen, seed=32):
    """unetdc_bn_eval_affine / unetdc_bn_frozen_affine: a sqrtf, a division or reciprocal and two products per channel."""
    c, eps = kw["c"], kw.get("eps", 1e-5)
    g = gen(seed)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) * 2 + 1e-3
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    ins = [vec(t) for t in (gamma, beta, rm, rv)]
    if frozen:
        outs = [outv(c) for _ in range(4)]
        call("unetdc_bn_frozen_affine", *(t.data_ptr() for t in ins), float(eps), *(o.view.data_ptr() for o in outs), c, stream())
        ref = X.bn_frozen_affine(gamma, beta, rm, rv, eps32)
        torch.cuda.synchronize()
        what = f"bn_frozen_affine(C {c})"
        check(outs[2], ref["mean"], 0, torch.float32, what + " mean")
        check(outs[3], ref["rstd"], 8 * E * ref["rstd"], torch.float32, what + " rstd")
        check(outs[0], ref["scale"], 10 * E * ref["scale"].abs(), torch.float32, what + " scale")
        check(outs[1], ref["shift"], 2 * E * ref["shift"].abs() + 14 * E * (ref["mean"] * ref["scale"]).abs(), torch.float32,
              what + " shift")
    else:
        bias = torch.randn(c, generator=g) if kw.get("ptr:conv_bias", True) else None
        outs = [outv(c) for _ in range(2)]
        bd = None if bias is None else vec(bias)
        call("unetdc_bn_eval_affine", *(t.data_ptr() for t in ins), None if bd is None else bd.data_ptr(), float(eps),
             outs[0].view.data_ptr(), outs[1].view.data_ptr(), c, stream())
        ref = X.bn_eval_affine(gamma, beta, rm, rv, eps32, bias)
        torch.cuda.synchronize()
        what = f"bn_eval_affine(C {c})"
        check(outs[0], ref["scale"], 8 * E * ref["scale"].abs(), torch.float32, what + " scale")
        d = (torch.zeros(c) if bias is None else bias).double() - rm.double()
        check(outs[1], ref["shift"], 2 * E * ref["shift"].abs() + 12 * E * (d * ref["scale"]).abs(), torch.float32,
              what + " shift")
    return None


# ---------------------------------------------------------------------------------------------------- BatchNorm backward
def bnbwd_fixture(n, h, w, c, g, pooled, skip, head=None, dev="cuda"):
    """Integer y in {-2..2}, integer shift / mean, power-of-two scale / rstd / gamma, gradients in {-1..1}: many exact
    scale * y + shift == 0 (the ReLU gate's edge) and many ties inside the 2x2 pool windows.  Returns the stored tensors and the
    constants (fp32)."""
    P = n * h * w
    y = X.ints((P, c), 2, dgen(g), device=dev)
    sc, sh = X.pow2(c, g, (-1, 0, 1)), X.ints((c,), 2, g)
    mu, rs = X.ints((c,), 1, g), X.pow2(c, g, (-1, 0))
    gamma = X.pow2(c, g, (-1, 0, 1)) * (1 - 2 * (torch.rand(c, generator=g) < 0.3).float())
    dskip = X.ints((P, c), 1, dgen(g), device=dev) if skip else None
    dpool = X.ints((P // 4, c), 1, dgen(g), device=dev) if pooled else None
    return y, dskip, dpool, (sc, sh, mu, rs, gamma)


def pre_parts_fixture(rows, c, g, dev="cuda"):
    """[rows, 3, C] partial sums as a producer leaves them: small integers, mostly zero."""
    p = X.ints((rows, 3, c), 3, dgen(g), device=dev)
    return torch.where(torch.rand(p.shape, generator=dgen(g), device=dev) < 0.3, p, torch.zeros_like(p))


def head_grad_fixture(n, h, w, g, oc=1, dev="cuda"):
    """Dyadic probabilities in {0, 1/4, 1/2, 3/4, 1} and integer dprobs in {-2..2} (one in eight nonzero): dz = dp p (1-p)
    is exact in fp32, in multiples of 1/16."""
    p = torch.randint(0, 5, (n, oc, h, w), generator=dgen(g), device=dev).float() / 4
    dp = X.ints((n, oc, h, w), 2, dgen(g), device=dev)
    dp = torch.where(torch.rand(dp.shape, generator=dgen(g), device=dev) < 0.125, dp, torch.zeros_like(dp))
    return dp, p


def bn_bwd_ref_check(ref, dyc, outs, dt, what, n, h, w, c, frozen=False):
    """dy under its fp32 bound; dgamma / dbeta (integer sums) equal at any count; dbias = -k3 S3 equal at a power-of-two count
    and in the frozen form (k1 S1: a power of two times an integer), else under exact_ref.bn_bwd_coeff_bounds."""
    check(dyc, ref["dy"], ref["dy_bound"], dt, what + " dy", (n, h, w, c))
    exact = frozen or pow2_count(n * h * w)
    for k, o in outs.items():
        if o is not None:
            check(o, ref[k], ref["dbias_bound"] if k == "dbias" and not exact else 0, torch.float32, f"{what} {k}")


def bn_relu_bwd(kw, variant="plain", seed=33):
    """unetdc_bn_relu_bwd / _frozen / _head.  kw: the header's names (n, h, w, c, dtype, lds, optional pointers, pre_nparts)."""
    n, h, w, c, dt = kw["n"], kw["h"], kw["w"], kw["c"], TD[kw["dtype"]]
    P = n * h * w
    head = variant == "head"
    pooled = kw.get("ptr:dpool", False)
    skip = kw.get("ptr:dskip", not pooled) and not head
    pre = kw.get("ptr:pre_parts", head)
    g = gen(seed)
    y, dskip, dpool, (sc, sh, mu, rs, gamma) = bnbwd_fixture(n, h, w, c, g, pooled, skip)
    T = conv_helpers()
    yc = T.put(y, kw.get("ldy", c + 64), dt)
    sc_, sh_, mu_, rs_, ga_ = (vec(t) for t in (sc, sh, mu, rs, gamma))
    dyc = T.out(P, c, kw.get("lddy", c + 32), dt)
    outs = {k: outv(c) for k in ("dgamma", "dbeta")}
    outs["dbias"] = outv(c) if kw.get("ptr:dbias", True) else None
    nbytes = lib().unetdc_bn_relu_bwd_workspace(n, h, w, c, int(pooled), kw["dtype"])
    ws = X.stats_guard(nbytes // 4)
    sums, pc, rows = None, None, 0
    if pre:
        rows = kw.get("pre_nparts") or lib().unetdc_conv3x3_stats_rows(P, c)
        pp = pre_parts_fixture(rows, c, g)
        sums = tuple(pp.double().sum(0))
        pc = X.stats_guard((rows + 64) * 3 * c)
        pc.view.view(-1)[: rows * 3 * c] = pp.reshape(-1)
    grad = dskip
    if head:
        dprobs, probs = head_grad_fixture(n, h, w, g)
        hw_ = X.ints((c,), 2, g) / 2
        grad = X.to_storage(X.head_dz(dprobs, probs).reshape(P, 1) * hw_.cuda().double(), dt).double()
        assert torch.equal(grad, X.head_dz(dprobs, probs).reshape(P, 1) * hw_.cuda().double()), "head gradient not exact"
        hd = [dprobs.contiguous(), probs.contiguous(), vec(hw_)]
        call("unetdc_bn_relu_bwd_head", *(t.data_ptr() for t in hd), yc.view.data_ptr(), yc.ld, sc_.data_ptr(), sh_.data_ptr(),
             mu_.data_ptr(), rs_.data_ptr(), ga_.data_ptr(), dyc.view.data_ptr(), dyc.ld, outs["dgamma"].view.data_ptr(),
             outs["dbeta"].view.data_ptr(), None if outs["dbias"] is None else outs["dbias"].view.data_ptr(), ws.view.data_ptr(),
             nbytes, pc.view.data_ptr(), rows, n, h, w, c, kw["dtype"], stream())
    else:
        dsc = T.put(dskip, kw.get("ldskip", 2 * c), dt) if skip else None
        dpc = T.put(dpool, kw.get("ldpool", c + 64), dt) if pooled else None
        call("unetdc_bn_relu_bwd_frozen" if variant == "frozen" else "unetdc_bn_relu_bwd",
             None if dsc is None else dsc.view.data_ptr(), 0 if dsc is None else dsc.ld,
             None if dpc is None else dpc.view.data_ptr(), 0 if dpc is None else dpc.ld, yc.view.data_ptr(), yc.ld,
             sc_.data_ptr(), sh_.data_ptr(), mu_.data_ptr(), rs_.data_ptr(), ga_.data_ptr(), dyc.view.data_ptr(), dyc.ld,
             outs["dgamma"].view.data_ptr(), outs["dbeta"].view.data_ptr(),
             None if outs["dbias"] is None else outs["dbias"].view.data_ptr(), ws.view.data_ptr(), nbytes,
             None if pc is None else pc.view.data_ptr(), rows, n, h, w, c, kw["dtype"], stream())
    torch.cuda.synchronize()
    v = lambda t: None if t is None else t.view(n, h, w, c)     # noqa: E731
    ref = X.bn_relu_bwd(v(y), sc, sh, mu, rs, gamma, v(grad), None if dpool is None else dpool.view(n, h // 2, w // 2, c), dt,
                        frozen=variant == "frozen", sums=sums)
    if sums is None:                              # the fp32 partial sums of the reduction pass must be exact
        for k, res in (("gh", 1.0), ("xh", 0.5)):
            assert X.sum_is_exact(ref[k].reshape(-1, c), res), k
        assert X.sum_is_exact((ref["gh"] * ref["xh"]).reshape(-1, c), 0.5), "gh * xh"
    what = f"bn_relu_bwd/{variant}(N {n}, {h}x{w}, C {c}, {dt}, {'pool' if pooled else ''}{'+skip' if skip else ''}" \
           f"{f', {rows} pre rows' if pre else ''})"
    bn_bwd_ref_check(ref, dyc, outs, dt, what, n, h, w, c, frozen=variant == "frozen")
    X.assert_guard(ws, what + " workspace")
    if pc is not None:
        X.assert_guard(pc, what + " pre_parts")
    return None


def bn_relu_bwd_coeffs(kw, seed=34):
    n, h, w, c = kw["n"], kw["h"], kw["w"], kw["c"]
    P = n * h * w
    g = gen(seed)
    rows = kw.get("pre_nparts") or lib().unetdc_conv3x3_stats_rows(P, c)
    pp = pre_parts_fixture(rows, c, g)
    pc = X.stats_guard((rows + 64) * 3 * c)
    pc.view.view(-1)[: rows * 3 * c] = pp.reshape(-1)
    rs, gamma = X.pow2(c, g, (-1, 0)), X.pow2(c, g, (-1, 0, 1))
    outs = {k: outv(c) for k in ("dgamma", "dbeta", "dbias")}
    co = outv(3 * c)
    ga_, rs_ = vec(gamma), vec(rs)
    call("unetdc_bn_relu_bwd_coeffs", pc.view.data_ptr(), rows, ga_.data_ptr(), rs_.data_ptr(), outs["dgamma"].view.data_ptr(),
         outs["dbeta"].view.data_ptr(), outs["dbias"].view.data_ptr(), co.view.data_ptr(), n, h, w, c, stream())
    torch.cuda.synchronize()
    s = pp.double().sum(0)
    k1 = gamma.double().cuda() * rs.double().cuda()
    k2, k3 = k1 * s[0] / P, k1 * s[1] / P
    ref = dict(dgamma=s[1], dbeta=s[0], dbias=-k3 * s[2], coeffs=torch.cat([k1, k2, k3]))
    what = f"bn_relu_bwd_coeffs(N {n}, {h}x{w}, C {c}, {rows} rows)"
    # k1 = gamma rstd is a power of two at any count; k2, k3 and dbias are exact at a power-of-two count only
    b = {k: torch.zeros_like(v) for k, v in X.bn_bwd_coeff_bounds(k2, k3, ref["dbias"]).items()} if pow2_count(P) \
        else X.bn_bwd_coeff_bounds(k2, k3, ref["dbias"])
    for k, o in outs.items():
        check(o, ref[k], b["dbias_bound"] if k == "dbias" else 0, torch.float32, f"{what} {k}")
    check(co, ref["coeffs"], torch.cat([torch.zeros_like(k1), b["k2_bound"], b["k3_bound"]]), torch.float32, what + " k1/k2/k3")
    X.assert_guard(pc, what + " pre_parts")
    return None


# ---------------------------------------------------------------------------------------------------- head
def head_fwd(kw, bn=False, seed=35):
    """unetdc_head_fwd (a stored) / unetdc_head_fwd_bn (relu(scale y + shift) on load): dyadic a and w, so z is exact and
    only expf, the add and the division round."""
    n, h, w, c, oc, dt = kw["n"], kw["h"], kw["w"], kw["c"], kw["oc"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    T = conv_helpers()
    wt, b = X.ints((oc, c), 2, g) / 16, X.ints((oc,), 4, g) / 4
    if bn:
        y = dints((P, c), 2, g)
        sc, sh = X.pow2(c, g, (-1, 0, 1)), X.ints((c,), 2, g)
        a = X.bn_relu(y, sc, sh)
        src = T.put(y, kw.get("ldy", c + 64), dt)
    else:
        a = dints((P, c), 2, g, lo=0).double()
        src = T.put(a.float(), kw.get("lda", c + 64), dt)
    pr = X.carve(n * oc, h * w, h * w, 0, torch.float32, MARGIN)
    wd_, bd = vec(wt.reshape(-1)), vec(b)
    if bn:
        scd, shd = vec(sc), vec(sh)
        call("unetdc_head_fwd_bn", src.view.data_ptr(), src.ld, scd.data_ptr(), shd.data_ptr(), wd_.data_ptr(), bd.data_ptr(),
             pr.view.data_ptr(), n, h, w, c, oc, kw["dtype"], stream())
    else:
        call("unetdc_head_fwd", src.view.data_ptr(), src.ld, wd_.data_ptr(), bd.data_ptr(), pr.view.data_ptr(), n, h, w, c, oc,
             kw["dtype"], stream())
    torch.cuda.synchronize()
    z, p = X.head_fwd(a, wt, b, n, h, w)
    dz = (c // 2 + 8) * E * (a.abs() @ wt.abs().double().cuda().t()).view(n, h, w, oc).permute(0, 3, 1, 2) + E * z.abs()
    bound = p * (1 - p) * (dz + 8 * E) + 4 * E * p
    check(pr, p.reshape(n * oc, h * w), bound.reshape(n * oc, h * w), torch.float32,
          f"head_fwd{'_bn' if bn else ''}(N {n}, {h}x{w}, C {c}, OC {oc}, {dt})")
    return None


def head_bwd(kw, bnstats=True, seed=36):
    """unetdc_head_bwd / unetdc_head_bwd_bnstats with dyadic probabilities and integer dprobs: dz, dW, db, dA and the
    BatchNorm sums are exact (asserted), so all of them are compared for equality."""
    n, h, w, c, oc, dt = kw["n"], kw["h"], kw["w"], kw["c"], kw["oc"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    T = conv_helpers()
    stored_a = kw.get("ptr:a", True) or not bnstats
    store_da = kw.get("ptr:da", True)
    dprobs, probs = head_grad_fixture(n, h, w, g, oc)
    wt = X.ints((oc, c), 2, g) / 2
    y = dints((P, c), 2, g)
    sc, sh = X.pow2(c, g, (-1, 0, 1)), X.ints((c,), 2, g)
    mu, rs = X.ints((c,), 1, g), X.pow2(c, g, (-1, 0))
    a = X.to_storage(X.bn_relu(y, sc, sh), dt).double()
    ref = X.head_bwd(dprobs, probs, a, wt, dt, bn=(y, sc, sh, mu, rs) if bnstats else None)
    dz = ref["dz"]
    assert X.sum_is_exact(dz, 1 / 16) and X.sum_is_exact(dz.unsqueeze(2) * a.unsqueeze(1), 1 / 32)
    assert torch.equal(X.to_storage(ref["da"], dt).double(), ref["da"]), "dA not exact in the storage type"
    ac = T.put(a.float(), kw.get("lda", c + 64), dt) if stored_a else None
    dac = T.out(P, c, kw.get("ldda", c + 32), dt) if store_da else None
    dwc, dbc = outv(oc * c), outv(oc)
    nbytes = lib().unetdc_head_bwd_workspace(n, h, w, c, oc, kw["dtype"])
    ws = X.stats_guard(nbytes // 4)
    wd_ = vec(wt.reshape(-1))
    common = (dprobs.data_ptr(), probs.data_ptr(), None if ac is None else ac.view.data_ptr(),
              64 if ac is None else ac.ld, wd_.data_ptr(), None if dac is None else dac.view.data_ptr(),
              c if dac is None else dac.ld, dwc.view.data_ptr(), dbc.view.data_ptr(), ws.view.data_ptr(), nbytes)
    what = f"head_bwd{'_bnstats' if bnstats else ''}(N {n}, {h}x{w}, C {c}, OC {oc}, {dt}, a {'stored' if stored_a else 'NULL'}, " \
           f"dA {'stored' if store_da else 'NULL'})"
    if bnstats:
        rows = lib().unetdc_conv3x3_stats_rows(P, c)
        pf = kw.get("parts_floats") or (rows + 64) * 3 * c
        parts = X.stats_guard(pf)
        npart = ctypes.c_int(-1)
        yc = T.put(y, kw.get("ldy_prev", c + 32), dt)
        cs = [vec(t) for t in (sc, sh, mu, rs)]
        call("unetdc_head_bwd_bnstats", *common, yc.view.data_ptr(), yc.ld, *(t.data_ptr() for t in cs), parts.view.data_ptr(),
             pf, ctypes.byref(npart), n, h, w, c, oc, kw["dtype"], stream())
        assert X.sum_is_exact(ref["xh"], 0.5) and X.sum_is_exact(ref["gh"], 1 / 32) and X.sum_is_exact(ref["gh"] * ref["xh"], 1 / 64)
    else:
        call("unetdc_head_bwd", *common, n, h, w, c, oc, kw["dtype"], stream())
    torch.cuda.synchronize()
    check(dwc, ref["dw"].reshape(-1), 0, torch.float32, what + " dW")
    check(dbc, ref["db"], 0, torch.float32, what + " db")
    if dac is not None:
        check(dac, ref["da"], 0, dt, what + " dA", (n, h, w, c))
    X.assert_guard(ws, what + " workspace")
    if bnstats:
        X.assert_guard(parts, what + " parts")
        k = npart.value
        assert 1 <= k and (k + 64) * 3 * c <= pf, (what, k)
        rows_ = parts.view.reshape(-1)[: k * 3 * c].view(k, 3, c)
        assert bool(torch.isfinite(rows_).all()), what + ": a parts row was not written"
        tot = rows_.double().sum(0)
        for i, s in enumerate(("s1", "s2", "s3")):
            check(tot[i], ref[s], 0, torch.float32, f"{what} BatchNorm sum {s.upper()}")
    return None


# ---------------------------------------------------------------------------------------------------- loss
EDGE_P = (0.0, 1.0, 1e-45, 1 - 2 ** -24)


def loss_fixture(nimg, hw, g):
    """Probabilities: uniform fp32 in (0, 1), a share of dyadic ones, and the edges {0, 1, 1e-45 (below the log clamp),
    1 - 2^-24}; binary targets with some soft ones."""
    p = torch.rand(nimg, hw, generator=dgen(g), device="cuda")
    k = torch.randint(0, 8, (nimg, hw), generator=dgen(g), device="cuda")
    edge = torch.tensor(EDGE_P, device="cuda", dtype=torch.float32)
    p = torch.where(k < 2, edge[torch.randint(0, 4, (nimg, hw), generator=dgen(g), device="cuda")], p)
    t = (torch.rand(nimg, hw, generator=dgen(g), device="cuda") < 0.3).float()
    t = torch.where(k == 7, torch.rand(nimg, hw, generator=dgen(g), device="cuda"), t)
    if hw >= 8:                                    # every edge with both targets in every map
        p[:, :8] = edge.repeat(2)
        t[:, :8] = torch.tensor([0.0] * 4 + [1.0] * 4, device="cuda")
    return p.contiguous(), t.contiguous()


def loss_nsum(hw):
    """Longest chain of fp32 additions behind one per-map partial sum of csrc/loss.hip: a lane's serial sum over
    ceil(hw / (blocks * 256)) elements (blocks = min(128, ceil(hw / 2048))), then 6 wave and 2 workgroup steps."""
    nb = min(128, max(1, math.ceil(hw / 2048)))
    return math.ceil(hw / (nb * 256)) + 8


def focal_dice_loss(kw, seed=37):
    """unetdc_focal_dice_loss_fwd, then _bwd with its coefficients; both compared with exact_ref.focal_dice_bounds."""
    nimg, hw = kw["nimg"], kw["hw"]
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))       # noqa: E731
    alpha, gamma, ratio, smooth = (f32(kw.get(k, d)) for k, d in (("alpha", 1.0), ("gamma", 2.0), ("ratio", 0.3), ("smooth", 1e-7)))
    gout = f32(kw.get("grad_out", 1.0))
    g = gen(seed)
    p, t = loss_fixture(nimg, hw, g)
    nbytes = lib().unetdc_focal_dice_loss_workspace(nimg, hw)
    ws = X.stats_guard(max(nbytes // 4, 1))
    lo, co = outv(1), outv(2 * nimg)
    call("unetdc_focal_dice_loss_fwd", p.data_ptr(), t.data_ptr(), lo.view.data_ptr(), co.view.data_ptr(), ws.view.data_ptr(),
         nbytes, nimg, hw, alpha, gamma, ratio, smooth, stream())
    go = torch.tensor([gout], device="cuda")
    dp = X.carve(nimg, hw, hw, 0, torch.float32, MARGIN)
    call("unetdc_focal_dice_loss_bwd", p.data_ptr(), t.data_ptr(), co.view.data_ptr(), go.data_ptr(), dp.view.data_ptr(), nimg, hw,
         alpha, gamma, ratio, stream())
    torch.cuda.synchronize()
    (llo, lhi), (dlo, dhi) = X.focal_dice_bounds(p, t, alpha, gamma, ratio, smooth, gout, loss_nsum(hw))
    what = f"focal_dice_loss(nimg {nimg}, hw {hw}, gamma {gamma}, grad_out {gout})"
    got = float(lo.view[0, 0])
    assert float(llo) <= got <= float(lhi), f"{what}: loss {got!r} outside [{float(llo)!r}, {float(lhi)!r}]"
    X.assert_guard(lo, what + " loss")
    X.assert_guard(co, what + " coef")
    X.assert_guard(ws, what + " workspace")
    mid, half = (dlo + dhi) / 2, (dhi - dlo) / 2
    check(dp, mid, half, torch.float32, what + " dprobs", (nimg, hw))
    return None


# ---------------------------------------------------------------------------------------------------- route cases
# channel counts of the network: 64..1024 -> C / EPC = 8..128 (bf16) and 16..256 (fp32): one or several workgroup rows per
# chunk lane set ('seg' = 256 splits) in bn_bwd_kernel; pixel counts are powers of two as at every stage of a batch of 1, 2,
# 4 or 8 square power-of-two images
BN_CASES = [(2, 16, 32, 64), (1, 32, 32, 128), (2, 8, 16, 256), (1, 8, 8, 512), (2, 4, 4, 1024), (8, 64, 64, 64)]
# the stages of a 32^2 step (--crop 32, --tile 32): 16 values per channel (the 2 x 2 bottleneck of a batch of 4), the first level
# of one image (pooled to 16 x 16) and its enc4 (4 x 4, pooled to 2 x 2)
BN_CASES += [(4, 2, 2, 1024), (1, 32, 32, 64), (1, 4, 4, 512)]


def levels(n, h, w):
    """The per-level (N, h, w, C) of a step on N images of h x w: 64 channels at full size ... 1024 at 1/16."""
    return [(n, h >> l, w >> l, 64 << l) for l in range(5)]


# Off the power-of-two grid (counts 3 * 2^k, 5 * 2^k, 15 * 2^k, 45, 120, 4): the ragged last batch of an epoch (3 x 512^2),
# 3 x 48 x 80 (45-pixel bottleneck, 3 x 3 x 5: below the 64-lane width, odd rows) and 2 x 96 x 160 (120-pixel bottleneck, below
# one 256-pixel block), 5 x 24 x 40 (4800 pixels: 18 full 256-pixel blocks and a partial one, an odd number of rows) and
# 1 x 2 x 2 (four samples per channel).
ODD_BN_CASES = levels(3, 512, 512) + levels(3, 48, 80) + levels(2, 96, 160) + [(5, 24, 40, 128), (1, 2, 2, 1024)]
SMALL_ODD_BN_CASES = [(1, 3, 3, 1024)]     # the 48^2 bottleneck of one image: nine samples per channel
ODD_BN_CASES += SMALL_ODD_BN_CASES
FINALIZE_CASES = [(1, 64, 64), (37, 1 << 12, 6), (512, 1 << 17, 64), (513, 1 << 17, 128), (8192, 1 << 21, 64),
                  (2048, 1 << 19, 1024)]
# (rows, count, C) at counts that are not powers of two; (12, 2880, 256), (19, 4800, 128) and (386, 3 * 2^15 + 300, 64): one row
# per 256-pixel block, the last one partial (64, 192 and 44 pixels: finalize_parts gives it the smaller share)
ODD_FINALIZE_CASES = [(3, 768, 64), (1, 45, 1024), (1, 120, 1024), (1, 4, 1024), (513, 3 * (1 << 15) + 256, 128),
                      (3072, 3 << 18, 64), (12, 2880, 256), (19, 4800, 128), (386, 3 * (1 << 15) + 300, 64), (577, 5 * 384 * 384, 64)]
# appended after both lists (the ids of the existing cases stay): 16 values per channel in one row (4 x 2 x 2 x 1024, 1 x 4 x 4 x 512),
# the four rows of one 32 x 32 x 64 map, and nine values per channel (the 3 x 3 bottleneck of one 48^2 image)
SMALL_FINALIZE_CASES = [(1, 16, 1024), (1, 16, 512), (4, 1024, 64), (1, 9, 1024)]


@pytest.mark.parametrize("case", FINALIZE_CASES + ODD_FINALIZE_CASES + SMALL_FINALIZE_CASES)
def test_exact_bn_finalize(case):
    rows, count, c = case
    bn_finalize(dict(rows=rows, count=count, c=c, eps=0.0, momentum=0.1))
    bn_finalize(dict(rows=rows, count=count, c=c, eps=1e-5, momentum=0.1, **{"ptr:running_mean": False}))


@pytest.mark.parametrize("c", [64, 100, 1024])
def test_bn_affines(c):
    bn_affine(dict(c=c, eps=1e-5), frozen=False)
    bn_affine(dict(c=c, eps=1e-5, **{"ptr:conv_bias": False}), frozen=False)
    bn_affine(dict(c=c, eps=1e-5), frozen=True)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("form", ["skip", "pool", "skip+pool", "frozen+skip", "frozen+pool"])
@pytest.mark.parametrize("case", BN_CASES)
def test_exact_bn_relu_bwd(case, form, dtype):
    n, h, w, c = case
    kw = dict(n=n, h=h, w=w, c=c, dtype=DTYPES[dtype], **{"ptr:dskip": "skip" in form, "ptr:dpool": "pool" in form})
    bn_relu_bwd(kw, "frozen" if form.startswith("frozen") else "plain")


BN_FORMS = ["skip", "pool", "skip+pool", "frozen+skip", "frozen+pool"]
# every form at every off-grid case, except the three pooled forms at (3, 3, 5, 1024) and at (1, 3, 3, 1024): a 2x2 max-pool needs
# even H and W, and the network never pools such a map (H and W are multiples of 16 and the 1/16 map is not pooled).  Nothing else
# is left out.
ODD_BN_ITEMS = [(case, form) for case in ODD_BN_CASES for form in BN_FORMS if not ("pool" in form and (case[1] % 2 or case[2] % 2))]
assert len(ODD_BN_ITEMS) == len(ODD_BN_CASES) * len(BN_FORMS) - 6


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case,form", ODD_BN_ITEMS)
def test_bn_relu_bwd_off_the_power_of_two_grid(case, form, dtype):
    """The same runner at pixel counts that are not powers of two (and at 4 samples per channel, 1 x 2 x 2, which is one):
    dgamma, dbeta, the partial rows and the frozen forms stay exact; dbias under exact_ref.bn_bwd_coeff_bounds (the runner
    chooses: equality at a power-of-two count), dy under the fp32 rule of exact_ref.bn_relu_bwd."""
    n, h, w, c = case
    kw = dict(n=n, h=h, w=w, c=c, dtype=DTYPES[dtype], **{"ptr:dskip": "skip" in form, "ptr:dpool": "pool" in form})
    bn_relu_bwd(kw, "frozen" if form.startswith("frozen") else "plain")


# (shape, rows): 300 rows (<= 512: read directly) and the unetdc_conv3x3_stats_rows count of a production map (thousands:
# through the fp32 pre-stage)
PRE_CASES = [((2, 16, 32, 64), "few"), ((1, 16, 16, 512), "few"), ((8, 512, 512, 64), "few"), ((8, 512, 512, 64), "production"),
             ((8, 256, 256, 128), "few"), ((8, 256, 256, 128), "production")]
# off the power-of-two grid.  "step": the unetdc_conv3x3_stats_rows count of that map whatever it is (3072 rows at
# 3 x 512^2 x 64, through the fp32 pre-stage; one partial row at 45 pixels); "few": 300 rows, as above
# (the cases of SMALL_ODD_BN_CASES go last, behind the "few" ones: that keeps the ids of the existing items and does nothing else)
ODD_PRE_CASES = [(c, "step") for c in ODD_BN_CASES if c not in SMALL_ODD_BN_CASES] \
    + [((3, 512, 512, 64), "few"), ((3, 3, 5, 1024), "few"), ((5, 24, 40, 128), "few")] + [(c, "step") for c in SMALL_ODD_BN_CASES]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case,rows", PRE_CASES + ODD_PRE_CASES)
def test_exact_bn_relu_bwd_pre_parts(case, rows, dtype):
    """The non-pooled form fed with a producer's partial rows: <= 512 rows read directly, thousands through the fp32 pre-stage
    (unetdc_conv3x3_stats_rows at 8 x 512^2), also through _coeffs and the head form."""
    n, h, w, c = case
    nrows = 300 if rows == "few" else lib().unetdc_conv3x3_stats_rows(n * h * w, c)
    if rows != "step":
        assert (nrows > 512) == (rows == "production"), nrows
    elif case == (3, 512, 512, 64):
        assert nrows > 512, nrows                 # the ragged batch's first level still goes through the pre-stage
    kw = dict(n=n, h=h, w=w, c=c, dtype=DTYPES[dtype], pre_nparts=nrows, **{"ptr:pre_parts": True, "ptr:dskip": True})
    bn_relu_bwd(kw, "plain")
    bn_relu_bwd(dict(kw, **{"ptr:dbias": False}), "frozen")
    bn_relu_bwd_coeffs(kw)
    if c == 64:
        bn_relu_bwd(dict(kw, **{"ptr:dskip": False}), "head")


HEAD_CASES = [(2, 16, 24, 64), (1, 40, 56, 32), (3, 8, 8, 128), (8, 512, 512, 64)]
# the head's maps of the ragged batch and of the odd geometries, a 45-pixel map (below the 64-lane width) and a 4-pixel one
HEAD_CASES += [(3, 512, 512, 64), (3, 48, 80, 64), (2, 96, 160, 64), (5, 24, 40, 128), (3, 3, 5, 64), (1, 2, 2, 64)]
HEAD_CASES += [(1, 32, 32, 64), (3, 48, 48, 64)]       # the head of one 32^2 crop and of three 48^2 tiles


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("oc", [1, 2])
@pytest.mark.parametrize("case", HEAD_CASES)
def test_exact_head(case, oc, dtype):
    n, h, w, c = case
    kw = dict(n=n, h=h, w=w, c=c, oc=oc, dtype=DTYPES[dtype])
    head_fwd(kw)
    head_fwd(kw, bn=True)
    head_bwd(kw, bnstats=False)
    head_bwd(kw)                                                       # a stored, dA stored
    head_bwd(dict(kw, **{"ptr:a": False}))                            # a recomputed from y
    if oc == 1:
        head_bwd(dict(kw, **{"ptr:a": False, "ptr:da": False}))      # the lean training form


LOSS_CASES = [(1, 1, 2.0, 1.0), (8, 1000, 2.0, 1.0), (9, 1000, 1.5, -1.75), (17, 4099, 2.0, 0.5), (8, 128 * 2048, 2.0, 1.0),
              (9, 128 * 2048 + 777, 1.5, 1.0), (2, 1 << 20, 2.0, 3.0), (17, 1, 1.5, 1.0)]
LOSS_CASES += [(1, 32 * 32, 2.0, 1.0), (3, 48 * 48, 2.0, 1.0)]      # one 32^2 crop (half a 2048-pixel block), three 48^2 maps


@pytest.mark.parametrize("case", LOSS_CASES)
def test_focal_dice_loss_bounded(case):
    nimg, hw, gamma, gout = case
    focal_dice_loss(dict(nimg=nimg, hw=hw, alpha=1.0, gamma=gamma, ratio=0.3, smooth=1e-7, grad_out=gout))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_bn_relu_bwd_head_is_bit_identical_to_the_stored_form(dtype):
    """include/unetdc_hip.h: unetdc_bn_relu_bwd_head (after head_bwd_bnstats with dA = NULL) is bit-identical to
    head_bwd_bnstats with dA stored followed by bn_relu_bwd with its sums -- at the training shape, realistic probabilities."""
    n, h, w, c = 8, 512, 512, 64
    dt, dti = TD[DTYPES[dtype]], DTYPES[dtype]
    P = n * h * w
    g = gen(38)
    T = conv_helpers()
    y = (torch.randn(P, c, generator=dgen(g), device="cuda") * 1.5).to(dt)
    sc, sh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    mu, rs, gamma = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) + 0.5
    probs = torch.sigmoid(torch.randn(n, 1, h, w, generator=dgen(g), device="cuda") * 2)
    dprobs = torch.randn(n, 1, h, w, generator=dgen(g), device="cuda") * 1e-6
    wt = torch.randn(1, c, generator=g) * 0.1
    cs = [vec(t) for t in (sc, sh, mu, rs, gamma)]
    wd_ = vec(wt.reshape(-1))
    rows = lib().unetdc_conv3x3_stats_rows(P, c)
    pf = (rows + 64) * 3 * c
    hb = lib().unetdc_head_bwd_workspace(n, h, w, c, 1, dti)
    bb = lib().unetdc_bn_relu_bwd_workspace(n, h, w, c, 0, dti)
    res = []
    for stored in (True, False):
        parts = torch.empty(pf, device="cuda")
        npart = ctypes.c_int(-1)
        da = torch.empty(P, c, dtype=dt, device="cuda") if stored else None
        dw, db = torch.empty(c, device="cuda"), torch.empty(1, device="cuda")
        ws = torch.empty(max(hb, bb), dtype=torch.uint8, device="cuda")
        call("unetdc_head_bwd_bnstats", dprobs.data_ptr(), probs.data_ptr(), None, 64, wd_.data_ptr(),
             None if da is None else da.data_ptr(), c, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), hb, y.data_ptr(), c,
             *(t.data_ptr() for t in cs[:4]), parts.data_ptr(), pf, ctypes.byref(npart), n, h, w, c, 1, dti, stream())
        dy = torch.empty(P, c, dtype=dt, device="cuda")
        dg, dbe, dbi = (torch.empty(c, device="cuda") for _ in range(3))
        tail = (y.data_ptr(), c, *(t.data_ptr() for t in cs), dy.data_ptr(), c, dg.data_ptr(), dbe.data_ptr(), dbi.data_ptr(),
                ws.data_ptr(), bb, parts.data_ptr(), npart.value, n, h, w, c, dti, stream())
        if stored:
            call("unetdc_bn_relu_bwd", da.data_ptr(), c, None, 0, *tail)
        else:
            call("unetdc_bn_relu_bwd_head", dprobs.data_ptr(), probs.data_ptr(), wd_.data_ptr(), *tail)
        torch.cuda.synchronize()
        res.append(dict(parts=parts[: npart.value * 3 * c].clone(), dw=dw, db=db, dy=dy, dgamma=dg, dbeta=dbe, dbias=dbi))
    for k in res[0]:
        a, b = res[0][k], res[1][k]
        assert a.shape == b.shape and bool(torch.isfinite(a.float()).all()), k
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), \
            f"{k}: {int((a != b).sum())} elements differ between the stored and the recomputed head gradient"
    assert float(res[0]["dgamma"].abs().max()) > 0
