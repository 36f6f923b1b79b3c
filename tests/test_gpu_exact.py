"""Exact-integer and out-of-view-write tests of every convolution route (tests/exact_ref.py explains the exactness rule).

Every output is compared element by element with the exact reference -- no tolerance -- and every byte of an output
buffer outside its view (padding columns, the other half of a concat buffer, margins, stats rows past the declared
size) must still hold the NaN guard pattern after the call.  Inputs sit at off > 0 in wider buffers whose unused bytes
hold a large finite sentinel: a read of the wrong columns or rows that reaches the arithmetic ruins the result.

Route cases: the operator shapes of tests/test_gpu_ops.py, dense and one-hot fixtures, both dtypes.  Production replay:
one training step (or eval forward) per configuration is recorded -- UNetDC(1, 1), and the configurations the entry points
and the benchmark run: UNetDC(3, 1) and UNet(3, 1) in both dtypes, ragged last batches, dL/dx -- and every distinct call
(symbol, shapes, lds, dtype, optional pointers) is replayed through the same symbol with fresh exact fixtures -- it must
reach the same kernel.  The BatchNorm, head and loss calls of the step are replayed through the runners of
tests/test_gpu_exact_norm.py."""
import ctypes
import re

import pytest
import torch

from tests import exact_ref as X

pytestmark = pytest.mark.gpu

from tests import test_gpu_exact_norm as N

if torch.cuda.is_available():
    from tests.test_gpu_ops import CONV_CASES
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd._lib import call
else:
    CONV_CASES = []

TD = {0: torch.float32, 1: torch.bfloat16}
MARGIN = 3                      # guard rows before and after every view
SUM_TOL = 4e-6                  # fp32 statistics / column / BatchNorm-backward sums: |err| <= SUM_TOL * sum|terms| (~64 ulp)
KERNELS = set()                 # unetdc_last_kernel() of every route-case call (coverage test at the end)


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return _lib.load()


def last_kernel():
    return lib().unetdc_last_kernel().decode()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def wide_range(k, wmax=2):
    """Largest r <= 255 with k * r * wmax < 2^24: dense activations this wide make most outputs need bf16 rounding (small
    integers are exact in bf16 and would hide a store that truncates), while staying exact in bf16 storage and fp32 sums."""
    return min(255, (X.EXACT_LIMIT - 1) // (k * wmax))


def big(shape, r, g, lo=None):
    """Integer fixture of activation size, drawn on the device (seeded from g).  The references run where their inputs are,
    in fp64: exact for integer data whatever computes it (tests/exact_ref.py)."""
    gd = torch.Generator(device="cuda").manual_seed(int(torch.randint(1 << 30, (1,), generator=g)))
    return X.ints(shape, r, gd, lo, device="cuda")


def put(data, ld, dt, off=None):
    """Input view holding `data` ([rows, cols]) at column ld - cols of a sentinel-filled buffer (of a buffer of >= 2 GiB only
    the view is written)."""
    rows, cols = data.shape
    huge = (rows + 2 * MARGIN) * ld * dt.itemsize >= 1 << 31
    c = X.carve(rows, cols, ld, ld - cols if off is None else off, dt, MARGIN, fill=None if huge else "sentinel")
    c.view.copy_(data.cuda().to(dt))
    return c


def out(rows, cols, ld, dt, off=None):
    return X.carve(rows, cols, ld, ld - cols if off is None else off, dt, MARGIN)


def dev(t):
    return t.float().contiguous().cuda()


def expect_equal(c, exp, dt, what, shape=None, route=None):
    """Output view == the storage rounding of the exact value, element by element (torch's round-to-nearest-even
    conversion, == exact_ref.round_bf16: tests/test_exact_ref_cpu.py), and nothing written outside the view."""
    want = exp.reshape(c.view.shape).to(torch.float32).cuda().to(dt)
    if not torch.equal(c.view, want):
        got = c.view.float().cpu().contiguous()
        want = want.float().cpu()
        msg = X.describe_mismatch(got.view(shape) if shape else got, want.view(shape) if shape else want, what, route)
        assert msg is None, msg
    X.assert_guard(c, what)


def expect_sums(got, terms, what):
    """fp32 sums (per channel) vs fp64 sums of exact terms [rows, C]."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: channel {int((~torch.isfinite(got)).nonzero()[0])} holds {got[~torch.isfinite(got)][0]} (not written?)"
    ref, scale = terms.sum(0).cpu(), terms.abs().sum(0).cpu()
    err = (got - ref).abs()
    bad = ~(err <= SUM_TOL * scale)                 # NaN-strict
    assert not bool(bad.any()), f"{what}: channel {int(bad.nonzero()[0])} off by {float(err.max())} (sum|terms| {float(scale.max())})"


# ---------------------------------------------------------------------------------------------------- runners
# kw: the header's argument names -> values (shapes, lds, dtype; 'ptr:<name>' = whether an optional pointer is given;
# 'workspace_bytes').  fix: 'dense' or 'onehot'.  Every runner returns the kernel the call reached.

def conv_fwd(kw, fix, seed=1):
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    affine, stats = kw.get("ptr:scale", False), kw.get("ptr:stats_part", True)
    if fix == "dense":
        x, wt, route = big((P, ci), wide_range(9 * ci), g), X.dense_conv3x3(co, ci, g), None
    else:
        x = big((P, ci), 2, g, lo=1)
        wt, route = X.onehot_conv3x3(co, ci)
    X.assert_exact(9 * ci, x.abs().max(), 2)
    x4 = x.view(n, h, w, ci)
    acc = X.conv3x3_fwd_onehot(x4, route, co, d) if route else X.conv3x3_fwd(x4, wt, d)
    bias = None if affine else X.ints((co,), 2, g)
    sc, sh = (X.pow2(co, g, (-1, 0, 1)), X.ints((co,), 2, g)) if affine else (None, None)
    exp = X.bn_relu(acc, sc, sh) if affine else acc.double() + bias.to(acc.device, torch.float64)
    xc = put(x, kw.get("ldx", ci + 64), dt)
    yc = out(P, co, kw.get("ldy", 2 * co), dt)
    wf = pack_conv(wt, dt)[0]
    rows = lib().unetdc_conv3x3_stats_rows(P, co)
    st = X.stats_guard((rows + 64) * 2 * co) if stats and not affine else None
    live = ctypes.c_int(-1)
    bd, scd, shd = (None if t is None else dev(t) for t in (bias, sc, sh))
    call("unetdc_conv3x3_fwd", xc.view.data_ptr(), xc.ld, wf.data_ptr(), ptr(bd), ptr(scd), ptr(shd), yc.view.data_ptr(), yc.ld,
         None if st is None else st.view.data_ptr(), ctypes.byref(live), n, h, w, ci, co, d, kw["dtype"], stream())
    name = last_kernel()
    expect_equal(yc, exp, dt, f"conv3x3_fwd[{name}]", (n, h, w, co), route)
    if st is not None:
        check_stats(st, rows, live.value, yc, co, f"conv3x3_fwd stats[{name}]")
    return name


def check_stats(st, rows, live, yc, co, what):
    torch.cuda.synchronize()
    X.assert_guard(st, what)
    part = st.view.cpu().reshape(-1)[: rows * 2 * co].view(rows, 2, co)
    if live >= 0:                                   # rows past the live count are declared zero
        assert 1 <= live <= rows, (what, live, rows)
        assert bool((part[live:] == 0).all()), f"{what}: declared zero rows {live}..{rows} are not zero"
    else:                                           # no live count: every declared row carries data
        live = rows
    bad = ~torch.isfinite(part[:live])
    assert not bool(bad.any()), f"{what}: partial row {int(bad.nonzero()[0][0])} not written"
    y = yc.view.double()
    tot = part.double().sum(0)
    expect_sums(tot[0], y, what + " sum")
    expect_sums(tot[1], y * y, what + " sum of squares")


def conv_fwd_bnin(kw, fix, seed=2):
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    act_out = kw.get("ptr:act_out", False)
    mode = lib().unetdc_conv3x3_bnin_supported(n, h, w, ci, co, d, kw["dtype"])
    assert mode >= (2 if act_out else 1), (kw, mode)
    g = gen(seed)
    s = X.pow2(ci, g, (0, 1))
    if fix == "dense":
        xr, t, wt, route = big((P, ci), 2, g), X.ints((ci,), 2, g), X.dense_conv3x3(co, ci, g), None
    else:
        xr, t = big((P, ci), 2, g, lo=1), X.ints((ci,), 1, g, lo=-2)        # relu clamps where s x + t <= 0
        wt, route = X.onehot_conv3x3(co, ci)
    act = X.bn_relu(xr, s, t)
    X.assert_exact(9 * ci, act.abs().max(), 2)
    a4 = act.view(n, h, w, ci)
    acc = X.conv3x3_fwd_onehot(a4, route, co, d) if route else X.conv3x3_fwd(a4, wt, d)
    bias = X.ints((co,), 2, g)
    xc = put(xr, kw.get("ldx", ci + 64), dt)
    yc = out(P, co, kw.get("ldy", 2 * co), dt)
    ac = out(P, ci, kw.get("ldact", ci + 32), dt) if act_out else None
    wf = pack_conv(wt, dt)[0]
    rows = lib().unetdc_conv3x3_stats_rows(P, co)
    st = X.stats_guard((rows + 64) * 2 * co)
    live = ctypes.c_int(-1)
    sd, td, bd = dev(s), dev(t), dev(bias)
    call("unetdc_conv3x3_fwd_bnin", xc.view.data_ptr(), xc.ld, sd.data_ptr(), td.data_ptr(), wf.data_ptr(), bd.data_ptr(),
         yc.view.data_ptr(), yc.ld, st.view.data_ptr(), ctypes.byref(live), None if ac is None else ac.view.data_ptr(),
         0 if ac is None else ac.ld, n, h, w, ci, co, d, kw["dtype"], stream())
    name = last_kernel()
    expect_equal(yc, acc.double() + bias.to(acc.device, torch.float64), dt, f"conv3x3_fwd_bnin[{name}]", (n, h, w, co), route)
    check_stats(st, rows, live.value, yc, co, f"conv3x3_fwd_bnin stats[{name}]")
    if ac is not None:
        expect_equal(ac, act, dt, f"conv3x3_fwd_bnin act_out[{name}]", (n, h, w, ci))
    return name


def conv_dgrad(kw, fix, variant, seed=3):
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    dy = big((P, co), wide_range(9 * co) if fix == "dense" else 2, g)
    wt, route = (X.dense_conv3x3(co, ci, g), None) if fix == "dense" else X.onehot_conv3x3(co, ci)
    X.assert_exact(9 * co, dy.abs().max(), 2)
    d4 = dy.view(n, h, w, co)
    exp = X.conv3x3_dgrad_onehot(d4, route, ci, d) if route else X.conv3x3_dgrad(d4, wt, d)
    dyc = put(dy, kw.get("lddy", co + 64), dt)
    dxc = out(P, ci, kw.get("lddx", ci + 32), dt)
    wd = pack_conv(wt, dt)[1]
    args = (dyc.view.data_ptr(), dyc.ld, wd.data_ptr(), dxc.view.data_ptr(), dxc.ld)
    tail = (n, h, w, ci, co, d, kw["dtype"], stream())
    extra = None
    if variant == "plain":
        call("unetdc_conv3x3_dgrad", *args, *tail)
    elif variant == "colsum":
        c0, c = kw.get("c0", 0), kw.get("c", ci // 2)
        cs = X.stats_guard(c)
        nb = max(lib().unetdc_conv3x3_dgrad_colsum_workspace(n, h, w, ci), kw.get("workspace_bytes", 0))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
        call("unetdc_conv3x3_dgrad_colsum", *args, cs.view.data_ptr(), c0, c, ws.data_ptr(), nb, *tail)
        extra = ("colsum", cs, c0, c)
    else:
        extra = bnstats_call("unetdc_conv3x3_dgrad_bnstats", args, tail, P, ci, dt, g, kw)
    name = last_kernel()
    expect_equal(dxc, exp, dt, f"conv3x3_dgrad/{variant}[{name}]", (n, h, w, ci), None)
    check_extra(extra, dxc, f"conv3x3_dgrad/{variant}[{name}]", name)
    return name


def bnstats_call(sym, args, tail, P, ci, dt, g, kw):
    """The BatchNorm-backward partial sums of the consuming stage, with exact constants: integer y_prev / shift / mean,
    power-of-two scale / rstd (gate and xhat are exact; the sums are compared with SUM_TOL)."""
    yp = big((P, ci), 2, g)
    sc, sh, mu, rs = X.pow2(ci, g, (-1, 0, 1)), X.ints((ci,), 2, g), X.ints((ci,), 1, g), X.pow2(ci, g, (-1, 0))
    ypc = put(yp, kw.get("ldy_prev", ci + 64), dt)
    rows = lib().unetdc_conv3x3_stats_rows(P, ci)
    parts = X.stats_guard((rows + 64) * 3 * ci)
    npart = ctypes.c_int(-1)
    dv = [dev(t) for t in (sc, sh, mu, rs)]
    call(sym, *args, ypc.view.data_ptr(), ypc.ld, *(t.data_ptr() for t in dv), parts.view.data_ptr(), (rows + 64) * 3 * ci,
         ctypes.byref(npart), *tail)
    return ("bnstats", parts, yp, (sc, sh, mu, rs), npart, rows, dv)


def check_extra(extra, dxc, what, kernel):
    if extra is None:
        return
    torch.cuda.synchronize()
    if extra[0] == "colsum":
        _, cs, c0, c = extra
        X.assert_guard(cs, what + " colsum")
        expect_sums(cs.view.cpu().reshape(-1), dxc.view.double()[:, c0:c0 + c], what + " colsum")
        return
    _, parts, yp, (sc, sh, mu, rs), npart, rows, _ = extra
    X.assert_guard(parts, what + " parts")
    ci = yp.shape[1]
    assert 1 <= npart.value <= rows + 64, (what, npart.value)
    rows_ = parts.view.cpu().reshape(-1)[: npart.value * 3 * ci].view(npart.value, 3, ci)
    bad = ~torch.isfinite(rows_)
    assert not bool(bad.any()), f"{what}: parts row {int(bad.nonzero()[0][0])} not written"
    pc = rows_.double().sum(0)
    dx, y = dxc.view.double(), yp.cuda().double()
    sc, sh, mu, rs = (t.cuda().double() for t in (sc, sh, mu, rs))
    gate = (y * sc + sh) > 0
    gh = torch.where(gate, dx, torch.zeros_like(dx))
    xh = (y - mu) * rs
    expect_sums(pc[0], gh, what + " S1")
    expect_sums(pc[1], gh * xh, what + " S2")
    if kernel.startswith("igemm_conv_kernel<"):   # the stand-alone reduction behind the first-generation kernel sums xhat
        expect_sums(pc[2], xh, what + " S3")
    else:                                         # the fused epilogues leave the third row zero (include/unetdc_hip.h)
        assert bool((rows_[:, 2] == 0).all()), f"{what}: third parts row is not zero"


def conv_wgrad(kw, fix, bnin=False, seed=4):
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    s = X.pow2(ci, g, (0, 1)) if bnin else None
    if fix == "dense":              # x, dy and (bnin) the shift in {-1..1}: relu(s x + t) <= 3
        x = big((P, ci), 1, g)
        t = X.ints((ci,), 1, g) if bnin else None
        dy = big((P, co), 1, g)
        xa = X.bn_relu(x, s, t) if bnin else x
        X.assert_exact(P, xa.abs().max(), 1)
        exp = X.conv3x3_wgrad(xa.view(n, h, w, ci), dy.view(n, h, w, co), d)
    else:                           # separable input x = a (x) u: nine matrix-vector products on the host
        if bnin:                    # a in {0, 1}, t <= 0: act = relu(s a u + t) = a relu(s u + t), mixed signs and clamps
            s = X.pow2(ci, g, (0, 1) if 2 * P * 2 < X.EXACT_LIMIT else (0,))
        r = X.value_range(P * int(s.max()) if bnin else P, 1)
        a = big((n, h, w), 1, g, lo=0 if bnin else -1)
        u = X.ints((ci,), r, g)
        t = X.ints((ci,), 0, g, lo=-2) if bnin else None
        dy = big((P, co), 1, g)
        x = (a.view(P, 1) * u.to(a.device).view(1, ci))
        exp = X.conv3x3_wgrad_separable(a, X.bn_relu(u, s, t) if bnin else u, dy.view(n, h, w, co), d)
    xc = put(x, kw.get("ldx", ci + 64), dt)
    dyc = put(dy, kw.get("lddy", co + 32), dt)
    dw = X.stats_guard(co * ci * 9)
    nb = max(lib().unetdc_conv3x3_wgrad_workspace(n, h, w, ci, co, kw["dtype"]), kw.get("workspace_bytes", 0))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    if bnin:
        sd, td = dev(s), dev(t)
        call("unetdc_conv3x3_wgrad_bnin", xc.view.data_ptr(), xc.ld, sd.data_ptr(), td.data_ptr(), dyc.view.data_ptr(), dyc.ld,
             dw.view.data_ptr(), ws.data_ptr(), nb, n, h, w, ci, co, d, kw["dtype"], stream())
    else:
        call("unetdc_conv3x3_wgrad", xc.view.data_ptr(), xc.ld, dyc.view.data_ptr(), dyc.ld, dw.view.data_ptr(), ws.data_ptr(), nb,
             n, h, w, ci, co, d, kw["dtype"], stream())
    name = last_kernel()
    expect_equal(dw, exp, torch.float32, f"conv3x3_wgrad{'_bnin' if bnin else ''}[{name}]", (co, ci, 3, 3))
    return name


def first_fwd(kw, fix, seed=5):
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    affine, stats = kw.get("ptr:scale", False), kw.get("ptr:stats_part", True)
    x = big((n, ci, h, w), 2, g, lo=1 if fix == "onehot" else None)
    wt, route = (X.dense_conv3x3(co, ci, g), None) if fix == "dense" else X.onehot_conv3x3(co, ci)
    acc = X.first_fwd(x, wt, d)
    bias = None if affine else X.ints((co,), 2, g)
    sc, sh = (X.pow2(co, g, (-1, 0, 1)), X.ints((co,), 2, g)) if affine else (None, None)
    exp = X.bn_relu(acc, sc, sh) if affine else acc.double() + bias.to(acc.device, torch.float64)
    xc = put(x.view(n * ci, h * w), h * w, torch.float32)
    yc = out(P, co, kw.get("ldy", co + 64), dt)
    rows = lib().unetdc_conv3x3_first_stats_rows(P, ci, co)
    st = X.stats_guard((rows + 64) * 2 * co) if stats and not affine else None
    wd_, bd, scd, shd = (None if t is None else dev(t) for t in (wt, bias, sc, sh))
    call("unetdc_conv3x3_first_fwd", xc.view.data_ptr(), wd_.data_ptr(), ptr(bd), ptr(scd), ptr(shd), yc.view.data_ptr(), yc.ld,
         None if st is None else st.view.data_ptr(), n, h, w, ci, co, d, kw["dtype"], stream())
    name = last_kernel()
    expect_equal(yc, exp, dt, f"first_fwd[{name}]", (n, h, w, co), route)
    if st is not None:
        check_stats(st, rows, -1, yc, co, f"first_fwd stats[{name}]")
    return name


def first_wgrad(kw, fix, seed=6):
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    r = X.value_range(P)
    x = big((n, ci, h, w), r, g, lo=0 if fix == "onehot" else None)
    dy = big((P, co), r, g)
    exp = X.first_wgrad(x, dy.view(n, h, w, co), d)
    xc = put(x.view(n * ci, h * w), h * w, torch.float32)
    dyc = put(dy, kw.get("lddy", co + 64), dt)
    dw = X.stats_guard(co * ci * 9)
    nb = max(lib().unetdc_conv3x3_first_wgrad_workspace(n, h, w, ci, co), kw.get("workspace_bytes", 0))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    call("unetdc_conv3x3_first_wgrad", xc.view.data_ptr(), dyc.view.data_ptr(), dyc.ld, dw.view.data_ptr(), ws.data_ptr(), nb,
         n, h, w, ci, co, d, kw["dtype"], stream())
    name = last_kernel()
    expect_equal(dw, exp, torch.float32, f"first_wgrad[{name}]", (co, ci, 3, 3))
    return name


def first_dgrad(kw, fix, seed=7):
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    dy = big((P, co), 2, g)
    wt = X.dense_conv3x3(co, ci, g) if fix == "dense" else X.onehot_conv3x3(co, ci)[0]
    exp = X.first_dgrad(dy.view(n, h, w, co), wt, d)
    dyc = put(dy, kw.get("lddy", co + 64), dt)
    dxc = out(n * ci, h * w, h * w, torch.float32)
    wd_ = dev(wt)
    call("unetdc_conv3x3_first_dgrad", dyc.view.data_ptr(), dyc.ld, wd_.data_ptr(), dxc.view.data_ptr(), n, h, w, ci, co, d,
         kw["dtype"], stream())
    name = last_kernel()
    expect_equal(dxc, exp.reshape(n * ci, h * w), torch.float32, f"first_dgrad[{name}]", (n, ci, h, w))
    return name


def first_wgrad_bn(kw, fix, seed=12):
    """The first layer's weight gradient with the BatchNorm + ReLU backward applied on load: dy = k1 [s y + t > 0] dz - k2
    - k3 xhat, xhat = (y - mean) rstd.  Integer y / dz / shift / mean / k2 / k3 and power-of-two scale / rstd / k1 make
    dy exact (and exactly representable in bf16), so dw is compared bit for bit."""
    n, h, w, ci, co, d, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], kw["dilation"], TD[kw["dtype"]]
    P = n * h * w
    assert lib().unetdc_conv3x3_first_wgrad_bn_supported(n, h, w, ci, co, d, kw["dtype"]) == 1, kw
    g = gen(seed)
    wide = 6 * P < X.EXACT_LIMIT                 # |dy| <= 6, else k1 = 1 and k3 = 0: |dy| <= 2
    x = big((n, ci, h, w), 1, g, lo=0 if fix == "onehot" else -1)
    dz, y = big((P, co), 1, g), big((P, co), 2, g)
    sc, sh = X.pow2(co, g, (-1, 0, 1)), X.ints((co,), 2, g)
    mu, rs = X.ints((co,), 1, g), X.pow2(co, g, (-1, 0))
    k1 = X.pow2(co, g, (0, 1) if wide else (0,))
    k2, k3 = X.ints((co,), 1, g), X.ints((co,), 1 if wide else 0, g)
    to = lambda t_: t_.to(y.device, torch.float64)    # noqa: E731
    gate = (y.double() * to(sc) + to(sh)) > 0
    dy = to(k1) * torch.where(gate, dz.double(), torch.zeros_like(y, dtype=torch.float64)) - to(k2) \
        - to(k3) * (y.double() - to(mu)) * to(rs)
    X.assert_exact(P, 1, dy.abs().max())
    exp = X.first_wgrad(x, dy.view(n, h, w, co), d)
    xc = put(x.view(n * ci, h * w), h * w, torch.float32)
    dzc = put(dz, kw.get("lddz", co + 64), dt)
    yc = put(y, kw.get("ldy", co + 32), dt)
    dw = X.stats_guard(co * ci * 9)
    nb = max(lib().unetdc_conv3x3_first_wgrad_workspace(n, h, w, ci, co), kw.get("workspace_bytes", 0))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    dv = [dev(t) for t in (sc, sh, mu, rs, torch.cat([k1, k2, k3]))]
    call("unetdc_conv3x3_first_wgrad_bn", xc.view.data_ptr(), dzc.view.data_ptr(), dzc.ld, yc.view.data_ptr(), yc.ld,
         *(t.data_ptr() for t in dv), dw.view.data_ptr(), ws.data_ptr(), nb, n, h, w, ci, co, d, kw["dtype"], stream())
    name = last_kernel()
    expect_equal(dw, exp, torch.float32, f"first_wgrad_bn[{name}]", (co, ci, 3, 3))
    return name


def convt_fwd(kw, fix, seed=8):
    n, h, w, ci, co, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    x = big((P, ci), 2, g, lo=1 if fix == "onehot" else None)
    wt = X.ints((ci, co, 2, 2), 2, g) if fix == "dense" else X.onehot_convT2x2(ci, co)
    bias = X.ints((co,), 2, g)
    exp = X.convT2x2_fwd(x.view(n, h, w, ci), wt, bias)
    xc = put(x, kw.get("ldx", ci + 64), dt)
    uc = out(4 * P, co, kw.get("ldup", 2 * co), dt, off=0)      # the first half of a concat buffer
    wf = pack_convt(wt, dt)[0]
    bd = dev(bias)
    call("unetdc_convT2x2_fwd", xc.view.data_ptr(), xc.ld, wf.data_ptr(), bd.data_ptr(), uc.view.data_ptr(), uc.ld, n, h, w, ci, co,
         kw["dtype"], stream())
    name = last_kernel()
    expect_equal(uc, exp, dt, f"convT2x2_fwd[{name}]", (n, 2 * h, 2 * w, co))
    return name


def convt_dgrad(kw, fix, bnstats=False, seed=9):
    n, h, w, ci, co, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    dup = big((4 * P, co), 2, g)
    wt = X.ints((ci, co, 2, 2), 2, g) if fix == "dense" else X.onehot_convT2x2(ci, co)
    exp = X.convT2x2_dgrad(dup.view(n, 2 * h, 2 * w, co), wt)
    dc = put(dup, kw.get("lddup", 2 * co), dt, off=0)
    dxc = out(P, ci, kw.get("lddx", ci + 32), dt)
    wd = pack_convt(wt, dt)[1]
    args = (dc.view.data_ptr(), dc.ld, wd.data_ptr(), dxc.view.data_ptr(), dxc.ld)
    tail = (n, h, w, ci, co, kw["dtype"], stream())
    extra = None
    if bnstats:
        extra = bnstats_call("unetdc_convT2x2_dgrad_bnstats", args, tail, P, ci, dt, g, kw)
    else:
        call("unetdc_convT2x2_dgrad", *args, *tail)
    name = last_kernel()
    expect_equal(dxc, exp, dt, f"convT2x2_dgrad{'_bnstats' if bnstats else ''}[{name}]", (n, h, w, ci))
    check_extra(extra, dxc, f"convT2x2_dgrad_bnstats[{name}]", name)
    return name


def convt_wgrad(kw, fix, seed=10):
    n, h, w, ci, co, dt = kw["n"], kw["h"], kw["w"], kw["cin"], kw["cout"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    r = X.value_range(P)
    x = big((P, ci), r, g, lo=0 if fix == "onehot" else None)
    dup = big((4 * P, co), r, g)
    exp = X.convT2x2_wgrad(x.view(n, h, w, ci), dup.view(n, 2 * h, 2 * w, co))
    xc = put(x, kw.get("ldx", ci + 64), dt)
    dc = put(dup, kw.get("lddup", 2 * co), dt, off=0)
    dw = X.stats_guard(ci * co * 4)
    nb = max(lib().unetdc_convT2x2_wgrad_workspace(n, h, w, ci, co, kw["dtype"]), kw.get("workspace_bytes", 0))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    call("unetdc_convT2x2_wgrad", xc.view.data_ptr(), xc.ld, dc.view.data_ptr(), dc.ld, dw.view.data_ptr(), ws.data_ptr(), nb,
         n, h, w, ci, co, kw["dtype"], stream())
    name = last_kernel()
    expect_equal(dw, exp, torch.float32, f"convT2x2_wgrad[{name}]", (ci, co, 2, 2))
    return name


def bn_relu_apply(kw, fix, seed=11):
    """relu(s y + t) with a power-of-two s and an integer t, and the 2x2 max-pool of the stored activation."""
    n, h, w, c, dt = kw["n"], kw["h"], kw["w"], kw["c"], TD[kw["dtype"]]
    P = n * h * w
    g = gen(seed)
    affine, pool, store = kw.get("ptr:scale", True), kw.get("ptr:pooled", True), kw.get("ptr:a", True)
    y = big((P, c), 2, g) if fix == "dense" else big((P, c), 2, g) * 64 + big((P, c), 1, g)
    sc, sh = X.pow2(c, g, (-1, 0, 1)), X.ints((c,), 2, g)
    a = X.bn_relu(y, sc, sh) if affine else y.double()
    yc = put(y, kw.get("ldy", c + 64), dt)
    ac = out(P, c, kw.get("lda", 2 * c), dt) if store else None
    pc = out(P // 4, c, kw.get("ldp", c + 32), dt) if pool else None
    scd, shd = (dev(sc), dev(sh)) if affine else (None, None)
    call("unetdc_bn_relu_apply", yc.view.data_ptr(), yc.ld, ptr(scd), ptr(shd), None if ac is None else ac.view.data_ptr(),
         0 if ac is None else ac.ld, None if pc is None else pc.view.data_ptr(), 0 if pc is None else pc.ld, n, h, w, c, kw["dtype"],
         stream())
    if ac is not None:
        expect_equal(ac, a, dt, "bn_relu_apply", (n, h, w, c))
    if pc is not None:
        stored = X.to_storage(a, dt).float().view(n, h, w, c)
        expect_equal(pc, X.maxpool2(stored), dt, "bn_relu_apply pooled", (n, h // 2, w // 2, c))
    return None


def ptr(t):
    return None if t is None else t.data_ptr()


def pack_conv(wt, dt):
    co, ci = wt.shape[:2]
    wd = dev(wt)
    wf = torch.empty(9 * co * ci, dtype=dt, device="cuda")
    wg = torch.empty(9 * co * ci, dtype=dt, device="cuda")
    call("unetdc_pack_conv3x3", wd.data_ptr(), wf.data_ptr(), wg.data_ptr(), co, ci, 1 if dt == torch.bfloat16 else 0, stream())
    return wf, wg


def pack_convt(wt, dt):
    ci, co = wt.shape[:2]
    wd = dev(wt)
    wf = torch.empty(4 * co * ci, dtype=dt, device="cuda")
    wg = torch.empty(4 * co * ci, dtype=dt, device="cuda")
    call("unetdc_pack_convT2x2", wd.data_ptr(), wf.data_ptr(), wg.data_ptr(), ci, co, 1 if dt == torch.bfloat16 else 0, stream())
    return wf, wg


# ---------------------------------------------------------------------------------------------------- route cases
FIXTURES = ["dense", "onehot"]
DTYPES = {"f32": 0, "bf16": 1}
ROUTE_CASES = list(CONV_CASES) + [
    (1, 9, 13, 64, 64, 1),       # M = 117, not a multiple of 16: bf16 on the 32x32x16 DMA kernel (igemm_dma.hip)
    (1, 264, 512, 64, 64, 2)]    # bf16, d = 2, H / d = 132 not a multiple of the lattice tile: the 16x16x32 halo kernel
# The stages of a 32^2 ... 96^2 step (train_DC_focal.py --crop, quantify_droplets_batch.py --tile) and of the 256^2 bottleneck.
# Dilation >= the map side: the eight off-centre taps read only padding (forward and input gradient reduce to the centre tap, the
# weight gradient writes exact zeros into eight of nine taps, rect_plan finds an empty rectangle).  M = N h w below or at one
# 16-row MFMA tile.  The persistent lattice kernel with 4 items on a grid of 4.  SMALL_ROUTES records the kernels reached.
SMALL_ROUTE_CASES = [
    (1, 2, 2, 1024, 1024, 16),   # bottleneck.3 of 1 x 32^2: M = 4
    (3, 2, 2, 512, 1024, 16),    # bottleneck.0 of 3 x 32^2: M = 12
    (4, 2, 2, 512, 1024, 16),    # M = 16, exactly one tile
    (3, 3, 3, 1024, 1024, 16),   # 48^2 bottleneck: M = 27, odd map
    (1, 4, 4, 512, 512, 8),      # enc4 of 32^2, d >= side: M = 16
    (3, 4, 4, 256, 512, 8),      # the same stage at batch 3: M = 48
    (2, 8, 8, 256, 256, 4),      # enc3 of 32^2: the valid rectangles are 4 x 4
    (2, 16, 16, 512, 1024, 16),  # 256^2 bottleneck: d equals the side, so the rectangles are empty
    (1, 32, 32, 64, 64, 1),      # lattice, 4 items
    (1, 32, 32, 128, 64, 1),     # dec1.0 of 32^2: two K chunks on 4 items
    (1, 32, 32, 128, 128, 1),    # dec2 of 64^2: wide lattice, 4 items
    (3, 64, 64, 64, 64, 1),      # 48 items, 3 images
    (2, 16, 16, 64, 128, 2)]     # enc2.0 of 32^2: 8-pixel sub-lattices, not the lattice route
# SMALL_ROUTES: the kernel every call of those cases reached on MI355X (unetdc_last_kernel(); both fixtures reach the same).
# fp32, every case: all six forward / input-gradient calls on igemm_dma_kernel<float, 4, 2, 2> -- igemm_dma_kernel<float, 4, 1, 2>
#   where the GEMM's N is 64 (forward of the three C_out = 64 cases, input gradient of the three C_in = 64 cases) -- and the
#   weight gradient on wgrad_dma_kernel<float, 4> (1 at 64 x 64 and 128 -> 64 and 64 -> 128 channels, 2 at 128 x 128).
# bf16:
#   (1, 2, 2, 1024, 1024, 16), (3, 2, 2, 512, 1024, 16), (3, 3, 3, 1024, 1024, 16)   [M % 16 != 0]
#       fwd store / stats / affine, dgrad plain / colsum / bnstats: igemm_dma_kernel<__bf16, 4, 2, 2>; wgrad: wgrad_dma_kernel<__bf16, 4>
#   (4, 2, 2, 512, 1024, 16), (1, 4, 4, 512, 512, 8), (3, 4, 4, 256, 512, 8)
#       all six: igemm_dma16_kernel<4, 2, 4> ring3; wgrad: wgrad_dma_kernel<__bf16, 4>
#   (2, 8, 8, 256, 256, 4)       all six: igemm_dma16_kernel<4, 2, 4> ring3; wgrad: wgrad_rect_kernel
#   (2, 16, 16, 512, 1024, 16)   all six: igemm_dma16_kernel<4, 2, 4> ring3 blocks16x16; wgrad: wgrad_dma_kernel<__bf16, 4>
#   (1, 32, 32, 64, 64, 1), (3, 64, 64, 64, 64, 1)
#       fwd store / stats / affine: igemm_lattice_kernel<4, 1, 4, 1, 0> / <.., 1> / <.., 2>; dgrad plain / colsum / bnstats:
#       igemm_lattice_kernel<4, 1, 4, 1, 0> / <.., 1> / <.., 4>; wgrad: wgrad_dma_kernel<__bf16, 1>
#   (1, 32, 32, 128, 64, 1)      fwd: as at 64 x 64 channels; dgrad plain / colsum / bnstats: igemm_lattice_kernel<4, 2, 4, 2, 0> /
#       igemm_lattice_wide_kernel<1> / igemm_lattice_wide_kernel<4>; wgrad: wgrad_dma_kernel<__bf16, 1>
#   (1, 32, 32, 128, 128, 1)     fwd store / stats / affine: igemm_lattice_kernel<4, 2, 4, 2, 0> / igemm_lattice_wide_kernel<1> /
#       igemm_lattice_wide_kernel<2>; dgrad: as at 128 -> 64; wgrad: wgrad_dma_kernel<__bf16, 2>
#   (2, 16, 16, 64, 128, 2)      fwd (all three): igemm_dma16_kernel<4, 2, 4> ring3; dgrad (all three): igemm_dma16_kernel<4, 1, 4>;
#       wgrad: wgrad_dma_kernel<__bf16, 1>
ROUTE_CASES += SMALL_ROUTE_CASES
WGRAD_CASES = [(2, 512, 256, 64, 64, 1), (1, 520, 512, 128, 64, 1), (4, 256, 256, 64, 128, 2), (2, 128, 128, 256, 128, 8),
               (8, 64, 64, 128, 256, 4), (5, 64, 64, 1024, 512, 1),                      # tap-fused (wgrad_fused.hip)
               (2, 32, 32, 256, 256, 16), (1, 16, 24, 256, 512, 8), (3, 24, 40, 512, 256, 16),    # valid rectangles (bf16)
               (2, 96, 80, 64, 64, 2)]                                                   # K split with a ragged last slice
BNIN_CASES = [(2, 256, 256, 64, 64, 1), (2, 64, 256, 64, 64, 2), (2, 128, 128, 128, 128, 1), (2, 64, 256, 128, 128, 2),
              (3, 64, 192, 128, 256, 1), (1, 128, 256, 256, 256, 1)]
CONVT_CASES = [(2, 8, 12, 128, 64), (1, 16, 16, 256, 128), (1, 4, 4, 1024, 512), (2, 32, 32, 256, 128), (1, 64, 64, 128, 64),
               (2, 16, 96, 512, 256), (1, 4, 32, 128, 64), (3, 8, 32, 128, 64)]
# up-convolutions from the 2 x 2, 3 x 3 and 6 x 6 bottlenecks of 32^2, 48^2 and 96^2 and upconv2 of 32^2: MODE_SHUFFLE with
# Wo % 16 != 0 leaves the dma16 route (SMALL_ROUTES records the kernels reached)
SMALL_CONVT_CASES = [(1, 2, 2, 1024, 512), (3, 3, 3, 1024, 512), (2, 6, 6, 1024, 512), (1, 8, 8, 256, 128)]
# reached on MI355X -- fp32, every case: fwd, dgrad and dgrad_bnstats on igemm_dma_kernel<float, 4, 2, 2>, wgrad on
# wgrad_dma_kernel<float, 4> (2 at 256 -> 128); bf16, the three 1024 -> 512 cases: fwd, dgrad and dgrad_bnstats on
# igemm_dma_kernel<__bf16, 4, 2, 2>, wgrad on wgrad_dma_kernel<__bf16, 4>; bf16 (1, 8, 8, 256, 128): fwd on
# igemm_dma_kernel<__bf16, 4, 2, 2>, dgrad and dgrad_bnstats on igemm_dma16_kernel<4, 2, 4> ring3, wgrad on wgrad_dma_kernel<__bf16, 2>
CONVT_CASES += SMALL_CONVT_CASES
FIRST_CASES = [(2, 24, 40, 1), (2, 64, 64, 2), (3, 10, 10, 1), (1, 8, 8, 1), (2, 96, 136, 1)]
FIRST_BN_CASES = [(2, 16, 24), (1, 64, 64), (3, 40, 96)]
ROUTE_RUN = []                  # route-case items run in this session (test_route_coverage needs all of them)


def dense_affordable(case, fix):
    """The dense fixture needs a full GEMM on the host: maps of >= 128K pixels run the one-hot fixture only (their routes'
    dense arithmetic is the same kernel code as at the smaller maps)."""
    if fix == "dense" and case[0] * case[1] * case[2] >= 131072:
        pytest.skip("large map: one-hot fixture only (host reference cost)")


def kwargs(case, dtype, **extra):
    n, h, w, cin, cout, d = case
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, dilation=d, dtype=DTYPES[dtype], **extra)


@pytest.mark.parametrize("fix", FIXTURES)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", ROUTE_CASES)
def test_exact_conv3x3_routes(case, dtype, fix):
    """conv3x3_fwd in store / stats / affine-ReLU modes, dgrad, dgrad_colsum, dgrad_bnstats and wgrad."""
    ROUTE_RUN.append(1)
    dense_affordable(case, fix)
    kw = kwargs(case, dtype)
    names = {}
    for tag, mode in (("store", {"ptr:stats_part": False}), ("stats", {"ptr:stats_part": True}), ("affine", {"ptr:scale": True})):
        names["fwd/" + tag] = conv_fwd(dict(kw, **mode), fix)
    for variant in ("plain", "colsum", "bnstats"):
        names["dgrad/" + variant] = conv_dgrad(kw, fix, variant)
    names["wgrad"] = conv_wgrad(kw, fix)
    KERNELS.update(names.values())
    planned_routes(case, dtype, fix, names)


def planned_routes(case, dtype, fix, names):
    """What the planning code implies for the kernels a route case reached (names: call -> unetdc_last_kernel()):
      - d >= a map side: a tap's valid rectangle is empty, rect_plan returns 0 (wgrad_rect.hip): never wgrad_rect_kernel;
      - the bf16 cases of SMALL_ROUTE_CASES with d = 1 on 32 x 32 and 64 x 64 maps ((W / d) % 32 == 0, (H / d) % 8 == 0):
        forward and input gradient on a lattice kernel (igemm_lattice_supported comes first in plan_igemm);
      - bf16 with M % 16 != 0: no 16-row tile route (dma16 needs M % 16 == 0, the lattice and halo kernels whole tiles;
        the 16x16x32 weight-gradient kernels need >= 32K pixels)."""
    n, h, w, _, _, d = case
    small = case in SMALL_ROUTE_CASES
    if small:
        print(f"\n[route {case} {dtype} {fix}] " + ", ".join(f"{k}: {v}" for k, v in names.items()))
    if d >= min(h, w):
        assert "wgrad_rect_kernel" not in names["wgrad"], (case, dtype, names)
    if small and dtype == "bf16" and d == 1 and (h, w) in ((32, 32), (64, 64)):
        for k, v in names.items():
            assert k == "wgrad" or "lattice" in v, (case, k, v)
    if dtype == "bf16" and (n * h * w) % 16:
        for k, v in names.items():
            assert not any(t in v for t in ("dma16", "16x16x32", "lattice", "halo")), (case, k, v)


@pytest.mark.parametrize("fix", FIXTURES)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", WGRAD_CASES)
def test_exact_wgrad_routes(case, dtype, fix):
    """Tap-fused, valid-rectangle and K-split weight gradients."""
    ROUTE_RUN.append(1)
    dense_affordable(case, fix)
    KERNELS.add(conv_wgrad(kwargs(case, dtype), fix))


@pytest.mark.parametrize("fix", FIXTURES)
@pytest.mark.parametrize("case", BNIN_CASES)
def test_exact_normalise_on_load(case, fix):
    """conv3x3_fwd_bnin with and without act_out, conv3x3_wgrad_bnin (bf16)."""
    ROUTE_RUN.append(1)
    kw = kwargs(case, "bf16")
    assert lib().unetdc_conv3x3_bnin_supported(*case, 1) > 0, case
    KERNELS.add(conv_fwd_bnin(kw, fix))
    if case[4] % 128 == 0:
        KERNELS.add(conv_fwd_bnin(dict(kw, **{"ptr:act_out": True}), fix))
    KERNELS.add(conv_wgrad(kw, fix, bnin=True))


@pytest.mark.parametrize("fix", FIXTURES)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", CONVT_CASES)
def test_exact_conv_transpose_routes(case, dtype, fix):
    ROUTE_RUN.append(1)
    n, h, w, cin, cout = case
    kw = dict(n=n, h=h, w=w, cin=cin, cout=cout, dtype=DTYPES[dtype])
    names = dict(fwd=convt_fwd(kw, fix), dgrad=convt_dgrad(kw, fix), dgrad_bnstats=convt_dgrad(kw, fix, bnstats=True),
                 wgrad=convt_wgrad(kw, fix))
    KERNELS.update(names.values())
    if case in SMALL_CONVT_CASES:
        print(f"\n[convT {case} {dtype} {fix}] " + ", ".join(f"{k}: {v}" for k, v in names.items()))
        if dtype == "bf16" and w % 16:                # plan_igemm: MODE_SHUFFLE with Wo % 16 != 0 (Wo = the input width) leaves dma16
            assert "dma16" not in names["fwd"], (case, names)


@pytest.mark.parametrize("fix", FIXTURES)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("shape", FIRST_CASES)
def test_exact_first_layer_routes(shape, cin, dtype, fix):
    ROUTE_RUN.append(1)
    n, h, w, d = shape
    kw = dict(n=n, h=h, w=w, cin=cin, cout=64, dilation=d, dtype=DTYPES[dtype])
    KERNELS.add(first_fwd(kw, fix))
    KERNELS.add(first_fwd(dict(kw, **{"ptr:scale": True}), fix))
    KERNELS.add(first_wgrad(kw, fix))
    KERNELS.add(first_dgrad(kw, fix))


@pytest.mark.parametrize("fix", FIXTURES)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", FIRST_BN_CASES)
def test_exact_first_layer_wgrad_bn_on_load(case, dtype, fix):
    """unetdc_conv3x3_first_wgrad_bn: one input channel, dilation 1 (the production first-layer weight gradient)."""
    ROUTE_RUN.append(1)
    n, h, w = case
    KERNELS.add(first_wgrad_bn(dict(n=n, h=h, w=w, cin=1, cout=64, dilation=1, dtype=DTYPES[dtype]), fix))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("case", [(2, 16, 24, 64), (1, 8, 8, 1024), (3, 4, 4, 256), (2, 64, 96, 128),
                                  (1, 32, 32, 64), (1, 4, 4, 512)])            # a 32^2 step: pooled to 16 x 16 and to 2 x 2
def test_exact_bn_relu_apply(case, pool, dtype):
    n, h, w, c = case
    bn_relu_apply(dict(n=n, h=h, w=w, c=c, dtype=DTYPES[dtype], **{"ptr:pooled": pool}), "dense")


# >= 2 GiB operands: the input is a channel slice of a buffer of 2^31 bytes (64 x 64 pixels, leading dimension HUGE_LD), more
# than the buffer descriptors of the DMA / lattice / halo kernels take, so every call below reaches a first-generation kernel
# (64-bit addressing; at bs 8 x 1024^2 bf16 the decoder's dec1.0 forward and weight gradient do).  Only the slice is filled.
HUGE_LD = {"f32": 131072, "bf16": 262144}


def huge(**kw):
    return dict(dict(n=1, h=64, w=64, cin=64, cout=64, dilation=1), **kw)


HUGE_CASES = {   # case -> (runner, kw, the leading dimension that is huge, kernel; {T}: __bf16 / float)
    "fwd_store_64": (lambda kw: conv_fwd(kw, "dense"), huge(**{"ptr:stats_part": False}), "ldx", "igemm_conv_kernel<{T}, 4, 1>"),
    "fwd_store_128": (lambda kw: conv_fwd(kw, "dense"), huge(cout=128, **{"ptr:stats_part": False}), "ldx",
                      "igemm_conv_kernel<{T}, 2, 2>"),
    "fwd_stats_64": (lambda kw: conv_fwd(kw, "dense"), huge(), "ldx", "igemm_conv_kernel<{T}, 4, 1>"),
    "fwd_stats_128": (lambda kw: conv_fwd(kw, "dense"), huge(cout=128), "ldx", "igemm_conv_kernel<{T}, 4, 1>"),  # BM = 256 rows
    "fwd_affine_64": (lambda kw: conv_fwd(kw, "dense"), huge(**{"ptr:scale": True}), "ldx", "igemm_conv_kernel<{T}, 4, 1>"),
    "fwd_affine_128": (lambda kw: conv_fwd(kw, "dense"), huge(cout=128, **{"ptr:scale": True}), "ldx",
                       "igemm_conv_kernel<{T}, 2, 2>"),
    "dgrad": (lambda kw: conv_dgrad(kw, "dense", "plain"), huge(), "lddy", "igemm_conv_kernel<{T}, 4, 1>"),
    "dgrad_colsum": (lambda kw: conv_dgrad(kw, "dense", "colsum"), huge(), "lddy", "igemm_conv_kernel<{T}, 4, 1>"),
    # the first-generation kernel has no BatchNorm-backward epilogue: plain dgrad, then the stand-alone reduction (abi.hip)
    "dgrad_bnstats": (lambda kw: conv_dgrad(kw, "dense", "bnstats"), huge(), "lddy", "igemm_conv_kernel<{T}, 4, 1>"),
    "wgrad_64": (lambda kw: conv_wgrad(kw, "dense"), huge(), "ldx", "wgrad_kernel<{T}, 1>"),
    "wgrad_128": (lambda kw: conv_wgrad(kw, "dense"), huge(cin=128, cout=128), "ldx", "wgrad_kernel<{T}, 2>"),
    "convT_fwd": (lambda kw: convt_fwd(kw, "dense"), huge(), "ldx", "igemm_conv_kernel<{T}, 2, 2>"),
    "convT_dgrad": (lambda kw: convt_dgrad(kw, "dense"), huge(h=32, w=32), "lddup", "igemm_conv_kernel<{T}, 4, 1>"),
    "convT_dgrad_bnstats": (lambda kw: convt_dgrad(kw, "dense", bnstats=True), huge(h=32, w=32), "lddup",
                            "igemm_conv_kernel<{T}, 4, 1>"),
}


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", list(HUGE_CASES))
def test_exact_first_generation_routes_at_2gib(case, dtype):
    ROUTE_RUN.append(1)
    run, kw, ld, kernel = HUGE_CASES[case]
    try:
        name = run(dict(kw, dtype=DTYPES[dtype], **{ld: HUGE_LD[dtype]}))
    finally:
        torch.cuda.empty_cache()
    assert name == kernel.format(T="__bf16" if dtype == "bf16" else "float"), (case, dtype, name)
    KERNELS.add(name)


# every kernel family the library contains (regular expressions over unetdc_last_kernel(); per dtype where both exist)
FAMILIES = [r"igemm_lattice_wide_kernel<1>$", r"igemm_lattice_wide_kernel<2>", r"igemm_lattice_wide_kernel<4>",
            r"igemm_lattice_wide_kernel<1> bnin", r"igemm_lattice_kernel<", r"igemm_dma16_kernel<.*blocks16x16",
            r"igemm_dma16_kernel<[^>]*>( ring3)?$", r"igemm_halo16_kernel<", r"igemm_halo_kernel<float",
            r"igemm_dma_kernel<__bf16", r"igemm_dma_kernel<float", r"igemm_conv_kernel<__bf16", r"igemm_conv_kernel<float",
            r"wgrad_kernel<__bf16", r"wgrad_kernel<float", r"wgrad_dma_kernel<__bf16", r"wgrad_dma_kernel<float",
            r"wgrad_ring_split_kernel<\d, 16x16x32>$", r"wgrad_ring_split_kernel<\d, 16x16x32> paired$",
            r"wgrad_ring_split_kernel<\d, 16x16x32>( paired)? bnin", r"wgrad_fused_split_kernel<16x16x32>$",
            r"wgrad_fused_split_kernel<16x16x32> paired", r"wgrad_ring_kernel<float", r"wgrad_fused_kernel<float",
            r"wgrad_rect_kernel", r"convt_wgrad_kernel", r"first_mfma_fwd_kernel<__bf16", r"first_mfma_fwd_kernel<float",
            r"first_mfma_wgrad_kernel<__bf16", r"first_mfma_wgrad_kernel<float", r"first_wgrad_rows_kernel<__bf16>$",
            r"first_wgrad_rows_kernel<float>$", r"first_wgrad_rows_kernel<__bf16> bn", r"first_wgrad_rows_kernel<float> bn",
            r"first_conv_wgrad_kernel<__bf16", r"first_conv_wgrad_kernel<float", r"first_conv_fwd_kernel<__bf16",
            r"first_conv_fwd_kernel<float", r"first_dgrad_kernel<__bf16", r"first_dgrad_kernel<float"]
ROUTE_ITEMS = lambda: 4 * (len(ROUTE_CASES) + len(WGRAD_CASES) + len(CONVT_CASES) + len(FIRST_BN_CASES)) \
    + 2 * len(BNIN_CASES) + 8 * len(FIRST_CASES) + 2 * len(HUGE_CASES)    # noqa: E731


def test_route_coverage():
    """The route cases above reached every kernel family the default build dispatches to."""
    if len(ROUTE_RUN) != ROUTE_ITEMS():           # it reads the kernels those items reached: a subset proves nothing
        pytest.skip(f"needs every route-case item in this session before it ({len(ROUTE_RUN)} of {ROUTE_ITEMS()} ran)")
    names = sorted(k for k in KERNELS if k)
    print("\n".join(["kernels reached:"] + names))
    missing = [f for f in FAMILIES if not any(re.search(f, k) for k in names)]
    assert not missing, (missing, names)
    for mode in (0, 1, 2, 4):                     # the narrow lattice kernel in every epilogue mode (4: BatchNorm-backward sums)
        assert any(k.startswith("igemm_lattice_kernel<") and f", {mode}>" in k for k in names), (mode, names)
    assert any(k.startswith("igemm_lattice_kernel<") and k.endswith("bnin") for k in names), names


# ---------------------------------------------------------------------------------------------------- production replay
RUNNERS = {
    "unetdc_conv3x3_fwd": lambda kw: conv_fwd(kw, "onehot"),
    "unetdc_conv3x3_fwd_bnin": lambda kw: conv_fwd_bnin(kw, "onehot"),
    "unetdc_conv3x3_dgrad": lambda kw: conv_dgrad(kw, "onehot", "plain"),
    "unetdc_conv3x3_dgrad_colsum": lambda kw: conv_dgrad(kw, "onehot", "colsum"),
    "unetdc_conv3x3_dgrad_bnstats": lambda kw: conv_dgrad(kw, "onehot", "bnstats"),
    "unetdc_conv3x3_wgrad": lambda kw: conv_wgrad(kw, "onehot"),
    "unetdc_conv3x3_wgrad_bnin": lambda kw: conv_wgrad(kw, "onehot", bnin=True),
    "unetdc_conv3x3_first_fwd": lambda kw: first_fwd(kw, "onehot"),
    "unetdc_conv3x3_first_wgrad": lambda kw: first_wgrad(kw, "onehot"),
    "unetdc_conv3x3_first_wgrad_bn": lambda kw: first_wgrad_bn(kw, "onehot"),
    "unetdc_conv3x3_first_dgrad": lambda kw: first_dgrad(kw, "onehot"),
    "unetdc_convT2x2_fwd": lambda kw: convt_fwd(kw, "onehot"),
    "unetdc_convT2x2_dgrad": lambda kw: convt_dgrad(kw, "onehot"),
    "unetdc_convT2x2_dgrad_bnstats": lambda kw: convt_dgrad(kw, "onehot", bnstats=True),
    "unetdc_convT2x2_wgrad": lambda kw: convt_wgrad(kw, "onehot"),
    "unetdc_bn_relu_apply": lambda kw: bn_relu_apply(kw, "onehot"),
    # BatchNorm, head and loss (tests/test_gpu_exact_norm.py): exact or fp64-bounded, no matrix-core kernel name
    "unetdc_bn_finalize": lambda kw: N.bn_finalize(kw),
    "unetdc_bn_eval_affine": lambda kw: N.bn_affine(kw, frozen=False),
    "unetdc_bn_frozen_affine": lambda kw: N.bn_affine(kw, frozen=True),
    "unetdc_bn_relu_bwd": lambda kw: N.bn_relu_bwd(kw, "plain"),
    "unetdc_bn_relu_bwd_frozen": lambda kw: N.bn_relu_bwd(kw, "frozen"),
    "unetdc_bn_relu_bwd_head": lambda kw: N.bn_relu_bwd(kw, "head"),
    "unetdc_bn_relu_bwd_coeffs": lambda kw: N.bn_relu_bwd_coeffs(kw),
    "unetdc_head_fwd": lambda kw: N.head_fwd(kw),
    "unetdc_head_fwd_bn": lambda kw: N.head_fwd(kw, bn=True),
    "unetdc_head_bwd": lambda kw: N.head_bwd(kw, bnstats=False),
    "unetdc_head_bwd_bnstats": lambda kw: N.head_bwd(kw),
    "unetdc_focal_dice_loss_fwd": lambda kw: N.focal_dice_loss(kw),
    "unetdc_focal_dice_loss_bwd": lambda kw: N.focal_dice_loss(kw),
}
# symbols a step may issue that the replay does not run, with the reason and the test that covers them
REPLAY_EXEMPT = {
    "unetdc_pack_many": "weight re-packing, not step arithmetic: tests/test_gpu_ops.py::test_pack_many_matches_per_layer_packers",
    "unetdc_adam_step": "the optimizer step, not convolution / BatchNorm arithmetic: fp64-bounded p, m, v and bit-exact packed "
                        "images in tests/test_gpu_exact_optim.py",
}
NON_CONV = {s for s in RUNNERS if not any(k in s for k in ("conv3x3", "convT2x2"))}


def cfg(dtype, bs, size=512, mode="train", arch="unetdc", cin=1, loss="focal", dx=False, adam=False):
    return dict(dtype=dtype, bs=bs, size=size, mode=mode, arch=arch, cin=cin, loss=loss, dx=dx, adam=adam)


# config -> what record_step runs.  mode: train = one training step; eval = an eval-mode forward (BatchNorm folded from the
# running statistics); frozen = eval mode under autograd (frozen statistics), forward and backward.  arch / cin: UNetDC or
# the plain UNet (all dilations 1) with 1 or 3 input channels; loss: focal_dice_loss or train.py's combined_loss (BCE + Dice,
# ATen ops); dx: the input requires grad (dL/dx through the first layer); adam: FusedAdam.step() after the backward.
REPLAY_CONFIGS = {"bf16_8x512": cfg("bf16", 8), "f32_8x512": cfg("f32", 8),
                  "bf16_4x1024": cfg("bf16", 4, 1024), "bf16_8x512_eval": cfg("bf16", 8, mode="eval"),
                  "bf16_8x512_frozen": cfg("bf16", 8, mode="frozen"),
                  # the entry points' and the benchmark's own configurations
                  "dc3_f32_8x512": cfg("f32", 8, cin=3, adam=True),                          # train_DC_focal.py defaults
                  "unet3_f32_8x512": cfg("f32", 8, arch="unet", cin=3, loss="bce_dice", adam=True),   # train.py defaults
                  "unet3_bf16_8x512": cfg("bf16", 8, arch="unet", cin=3, adam=True),         # bench.py --arch unet
                  "dc3_f32_8x512_eval": cfg("f32", 8, mode="eval", cin=3),                  # quantify_droplets_batch.py
                  "dc3_bf16_8x512_eval": cfg("bf16", 8, mode="eval", cin=3),                # bench.py --mode quantify
                  # the ragged last batch of every epoch (the loaders have no drop_last)
                  "dc3_bf16_1x512": cfg("bf16", 1, cin=3, adam=True), "dc3_bf16_3x512": cfg("bf16", 3, cin=3, adam=True),
                  "dc3_f32_1x512": cfg("f32", 1, cin=3, adam=True), "dc3_f32_3x512": cfg("f32", 3, cin=3, adam=True),
                  # dL/dx at the production shape: the first layer's input-gradient kernel
                  "dc3_bf16_8x512_dx": cfg("bf16", 8, cin=3, dx=True), "dc3_f32_8x512_dx": cfg("f32", 8, cin=3, dx=True),
                  # train_DC_focal.py --img_size 384 --batch 5 --dtype bf16: no pixel count of the step is a power of two
                  # (5 * 9 * 2^k: 737280 ... 2880), maps of 384, 192, 96, 48 and 24 pixels a side (see the test's docstring)
                  "dc3_bf16_5x384": cfg("bf16", 5, 384, cin=3, adam=True),
                  # train_DC_focal.py --device_data --crop S: a full batch of the smallest crop in both dtypes, its ragged last
                  # batch (a 2 x 2 bottleneck: M = 4), and crops of 64 and 96
                  "crop_bf16_4x32": cfg("bf16", 4, 32, cin=3, adam=True), "crop_f32_4x32": cfg("f32", 4, 32, cin=3, adam=True),
                  "crop_bf16_1x32": cfg("bf16", 1, 32, cin=3, adam=True), "crop_bf16_3x64": cfg("bf16", 3, 64, cin=3, adam=True),
                  "crop_bf16_2x96": cfg("bf16", 2, 96, cin=3, adam=True),
                  # quantify_droplets_batch.py --tile T: a full chunk, the ragged last chunk of a 4 + 2 tile plan
                  # (tests/test_gpu_tiling.py), and the smallest tile
                  "tile_bf16_4x64_eval": cfg("bf16", 4, 64, mode="eval", cin=3),
                  "tile_bf16_2x48_eval": cfg("bf16", 2, 48, mode="eval", cin=3),
                  "tile_f32_4x48_eval": cfg("f32", 4, 48, mode="eval", cin=3),
                  "tile_bf16_1x32_eval": cfg("bf16", 1, 32, mode="eval", cin=3)}
# 1024^2: the forward and weight-gradient convolution calls and every non-convolution call (the host reference of the
# whole step is over the time budget; its input-gradient calls take the same kernels as at 512^2 with twice the items per
# workgroup)
REPLAY_ONLY = {"bf16_4x1024": ("fwd", "wgrad")}
# (batch 3 and 5 x 384^2: every pixel count is 3 * 2^k or 45 * 2^k; the BatchNorm runners of tests/test_gpu_exact_norm.py take any
# count -- sums and statistics stay exact, k2 / k3 / dbias are fp64-bounded there -- so every call of those steps is replayed)
# The kernels each native-resolution config reached on MI355X, as test_production_step_replay prints them (sym: kernels).
# crop_bf16_4x32   conv3x3_fwd: dma16<4, 2, 4> ring3, lattice<4, 1, 4, 1, 1>; conv3x3_dgrad: dma16<4, 1, 4>, dma16<4, 2, 4> ring3;
#   conv3x3_dgrad_bnstats: dma16<4, 2, 4> ring3, lattice<4, 1, 4, 1, 4>; conv3x3_dgrad_colsum: dma16<4, 2, 4> ring3, lattice_wide<1>;
#   conv3x3_wgrad: wgrad_dma<__bf16, 1 | 2 | 4>, wgrad_rect; convT2x2_fwd: dma16<4, 2, 4> ring3, igemm_dma<__bf16, 4, 2, 2>;
#   convT2x2_dgrad_bnstats: dma16<4, 2, 4> ring3; convT2x2_wgrad: wgrad_dma<__bf16, 1 | 2 | 4>; first_fwd / first_wgrad:
#   first_mfma_fwd_kernel<__bf16> / first_mfma_wgrad_kernel<__bf16> (so in every bf16 config below)
# crop_f32_4x32    conv3x3_fwd, conv3x3_dgrad, conv3x3_dgrad_bnstats: igemm_dma<float, 4, 1, 2>, igemm_dma<float, 4, 2, 2>;
#   conv3x3_dgrad_colsum, convT2x2_fwd, convT2x2_dgrad_bnstats: igemm_dma<float, 4, 2, 2>; conv3x3_wgrad, convT2x2_wgrad:
#   wgrad_dma<float, 1 | 2 | 4>; first_mfma_fwd_kernel<float>, first_mfma_wgrad_kernel<float>
# crop_bf16_1x32   as crop_bf16_4x32, plus igemm_dma<__bf16, 4, 2, 2> under conv3x3_fwd, conv3x3_dgrad, conv3x3_dgrad_bnstats and
#   convT2x2_dgrad_bnstats (the 2 x 2 bottleneck: M = 4)
# crop_bf16_3x64   conv3x3_fwd: dma16<4, 2, 4> ring3, lattice<4, 1, 4, 1, 1>, lattice_wide<1>; conv3x3_fwd_bnin: lattice_wide<1> bnin;
#   conv3x3_dgrad: dma16<4, 1, 4>, dma16<4, 2, 4> ring3; conv3x3_dgrad_bnstats: dma16<4, 2, 4> ring3, lattice<4, 1, 4, 1, 4>,
#   lattice_wide<4>; conv3x3_dgrad_colsum: dma16<4, 2, 4> ring3, lattice_wide<1>; conv3x3_wgrad: wgrad_dma<__bf16, 1 | 2 | 4>,
#   wgrad_rect; convT2x2_fwd: dma16<4, 2, 4> ring3, igemm_dma<__bf16, 4, 2, 2>; convT2x2_dgrad_bnstats: dma16<4, 2, 4> ring3;
#   convT2x2_wgrad: convt_wgrad_kernel, wgrad_dma<__bf16, 2 | 4>
# crop_bf16_2x96   the same lists as crop_bf16_1x32 (the 6 x 6 bottleneck: M = 72)
# tile_bf16_4x64_eval   conv3x3_fwd: dma16<4, 2, 4> ring3, lattice<4, 1, 4, 1, 2>, lattice_wide<2>; convT2x2_fwd: dma16<4, 2, 4> ring3,
#   igemm_dma<__bf16, 4, 2, 2>
# tile_bf16_2x48_eval   conv3x3_fwd: dma16<4, 1, 4>, dma16<4, 2, 4> ring3, igemm_dma<__bf16, 4, 2, 2>; convT2x2_fwd: igemm_dma<__bf16, 4, 2, 2>
# tile_f32_4x48_eval    conv3x3_fwd: igemm_dma<float, 4, 1, 2>, igemm_dma<float, 4, 2, 2>; convT2x2_fwd: igemm_dma<float, 4, 2, 2>
# tile_bf16_1x32_eval   conv3x3_fwd: dma16<4, 2, 4> ring3, igemm_dma<__bf16, 4, 2, 2>, lattice<4, 1, 4, 1, 2>; convT2x2_fwd: the call of
#   crop_bf16_1x32 (igemm_dma<__bf16, 4, 2, 2>, dma16<4, 2, 4> ring3)
# (dma16 = igemm_dma16_kernel, lattice = igemm_lattice_kernel, lattice_wide = igemm_lattice_wide_kernel, igemm_dma = igemm_dma_kernel,
#  wgrad_dma = wgrad_dma_kernel, wgrad_rect = wgrad_rect_kernel)
# kernels the native-resolution configs must reach, per symbol (test_production_step_replay's docstring says why)
REPLAY_NAMED = {
    # first reached by this config: wgrad_dma_kernel<__bf16, 1> under the 3x3 weight gradient, <__bf16, 1> and <__bf16, 2> under the
    # up-convolution's; also pinned: the lattice kernels on 16 items and enc3's valid-rectangle weight gradient
    "crop_bf16_4x32": {"unetdc_conv3x3_wgrad": ["wgrad_dma_kernel<__bf16, 1>", "wgrad_rect_kernel"],
                       "unetdc_convT2x2_wgrad": ["wgrad_dma_kernel<__bf16, 1>", "wgrad_dma_kernel<__bf16, 2>"],
                       "unetdc_conv3x3_fwd": ["igemm_lattice_kernel<4, 1, 4, 1, 1>"],
                       "unetdc_conv3x3_dgrad_bnstats": ["igemm_lattice_kernel<4, 1, 4, 1, 4>"]},
    # first reached by this config: all three pairs
    "crop_f32_4x32": {"unetdc_conv3x3_fwd": ["igemm_dma_kernel<float, 4, 1, 2>"],
                      "unetdc_conv3x3_dgrad_bnstats": ["igemm_dma_kernel<float, 4, 1, 2>"],
                      "unetdc_conv3x3_wgrad": ["wgrad_dma_kernel<float, 1>"]},
    "crop_bf16_1x32": {"unetdc_conv3x3_fwd": ["igemm_dma_kernel<__bf16, 4, 2, 2>"],
                       "unetdc_conv3x3_dgrad_bnstats": ["igemm_dma_kernel<__bf16, 4, 2, 2>"],
                       "unetdc_convT2x2_dgrad_bnstats": ["igemm_dma_kernel<__bf16, 4, 2, 2>"]},
    "crop_bf16_3x64": {"unetdc_conv3x3_fwd_bnin": ["igemm_lattice_wide_kernel<1> bnin"],
                       "unetdc_conv3x3_dgrad_bnstats": ["igemm_lattice_wide_kernel<4>"],
                       "unetdc_convT2x2_wgrad": ["convt_wgrad_kernel"]},
    "crop_bf16_2x96": {"unetdc_conv3x3_fwd": ["igemm_dma_kernel<__bf16, 4, 2, 2>"],
                       "unetdc_conv3x3_dgrad": ["igemm_dma_kernel<__bf16, 4, 2, 2>"]},
    "tile_bf16_4x64_eval": {"unetdc_conv3x3_fwd": ["igemm_lattice_kernel<4, 1, 4, 1, 2>", "igemm_lattice_wide_kernel<2>"]},
    "tile_bf16_2x48_eval": {"unetdc_conv3x3_fwd": ["igemm_dma_kernel<__bf16, 4, 2, 2>", "igemm_dma16_kernel<4, 1, 4>"]},
    "tile_f32_4x48_eval": {"unetdc_conv3x3_fwd": ["igemm_dma_kernel<float, 4, 1, 2>", "igemm_dma_kernel<float, 4, 2, 2>"]},
    "tile_bf16_1x32_eval": {"unetdc_conv3x3_fwd": ["igemm_lattice_kernel<4, 1, 4, 1, 2>", "igemm_dma_kernel<__bf16, 4, 2, 2>"]},
}
REPLAYED = set()                # distinct calls replayed by an earlier config of this session (not replayed again)


def record_step(dtype, bs, size, mode="train", arch="unetdc", cin=1, loss="focal", dx=False, adam=False):
    from models.model import UNet
    from models.model_2 import UNetDC
    from oracle import recipe
    from unet_dc_segmentation_amd.optim import FusedAdam
    from utils.metrics_DC import combined_loss, focal_dice_loss
    torch.manual_seed(5)
    model = (UNetDC if arch == "unetdc" else UNet)(cin, 1).cuda()
    model.train(mode == "train")
    if dtype == "bf16":
        model.set_compute_dtype("bf16")
    x = recipe.seeded_input(8, (bs, cin, size, size)).cuda()
    t = recipe.seeded_target(9, (bs, 1, size, size), frac=0.1).cuda()
    if dx:
        x.requires_grad_()
    opt = FusedAdam(model) if adam else None
    _lib.start_timing(_lib.SIGNATURES)            # every ABI name: the completeness check sees whatever the step issued
    try:
        if mode == "eval":
            with torch.no_grad():
                model(x)
        else:
            p = model(x)
            (focal_dice_loss(p, t, alpha=1.0, gamma=2.0, ratio=0.3) if loss == "focal" else combined_loss(p, t)).backward()
            if dx:
                assert x.grad is not None and bool(torch.isfinite(x.grad).all())
            if opt is not None:
                opt.step()
    finally:
        recs = _lib.stop_timing()
    del model, x, t, opt
    torch.cuda.empty_cache()
    return recs


def distinct_calls(recs):
    """(symbol, shapes, lds, dtype, scalar parameters, optional pointers given) -> (kw, recorded kernel): one replay per
    distinct call.  Symbols outside the argument table are returned by name with no kw."""
    out = {}
    for name_kernel, args, _ in recs:
        sym, kernel = name_kernel.split("|", 1)
        if sym not in X.ARGS:
            out.setdefault((sym,), (None, kernel))
            continue
        kinds = X.arg_kinds(_lib.SIGNATURES[sym][1])
        kw = {}
        for key, i in X.positions(sym, kinds).items():
            kw[key] = (args[i] is not None) if key.startswith("ptr:") else args[i]
        key = (sym,) + tuple(sorted((k, v) for k, v in kw.items() if k != "workspace_bytes"))
        if key not in out:
            out[key] = (kw, kernel)
        elif "workspace_bytes" in kw:
            out[key][0]["workspace_bytes"] = max(out[key][0]["workspace_bytes"], kw["workspace_bytes"])
    return out


@pytest.mark.parametrize("config", list(REPLAY_CONFIGS))
def test_production_step_replay(config):
    """Every distinct call of one training step (or eval forward, or frozen-statistics step), replayed with exact fixtures
    at its own shapes and leading dimensions: the same kernel, a bit-exact (or fp64-bounded) output, intact guards.  Every
    symbol the step issued has a runner or a named exemption.

    dc3_bf16_5x384 (train_DC_focal.py --img_size 384 --batch 5 --dtype bf16) reaches, where neither the 8 x 512^2 nor the
    3 x 512^2 bf16 step does: the first-generation DMA kernel in bf16 (igemm_dma_kernel<__bf16, 4, 2, 2>) for the
    up-convolution of the 24 x 24 bottleneck, wgrad_dma_kernel<__bf16, 4> for that up-convolution's weight gradient and
    wgrad_dma_kernel<__bf16, 2> for a 3x3 one, and igemm_dma16_kernel<4, 2, 4> ring3 under unetdc_conv3x3_dgrad_colsum (at
    512^2 every column-sum call takes the wide lattice kernel); its BatchNorm, head and loss calls run at counts 45 * 2^k.

    The native-resolution configs (--crop, --tile), in the order above; "new" = a (symbol, kernel) pair no earlier config
    replays, measured on MI355X.  crop_bf16_4x32 is the first to reach wgrad_dma_kernel<__bf16, 1> under unetdc_conv3x3_wgrad
    and wgrad_dma_kernel<__bf16, 1> / <__bf16, 2> under unetdc_convT2x2_wgrad; its 32 x 32 level runs the lattice kernels on 16
    items and enc3's 8 x 8 maps take wgrad_rect_kernel.  crop_f32_4x32 is the first to reach igemm_dma_kernel<float, 4, 1, 2>
    under unetdc_conv3x3_fwd and unetdc_conv3x3_dgrad_bnstats and wgrad_dma_kernel<float, 1> under unetdc_conv3x3_wgrad.
    crop_bf16_1x32 (M = 4 at the bottleneck) is the first to reach igemm_dma_kernel<__bf16, 4, 2, 2> under unetdc_conv3x3_fwd,
    unetdc_conv3x3_dgrad, unetdc_conv3x3_dgrad_bnstats and unetdc_convT2x2_dgrad_bnstats.  crop_bf16_3x64, crop_bf16_2x96 and the
    four eval configs reach no new pair: they replay known kernels at maps nothing replayed before -- crop_bf16_3x64 the
    normalise-on-load forward igemm_lattice_wide_kernel<1> bnin and convt_wgrad_kernel at 3 x 32 x 32, crop_bf16_2x96 and
    tile_bf16_2x48_eval the bottlenecks of 72 and 18 pixels (M % 16 != 0) on igemm_dma_kernel<__bf16, 4, 2, 2>,
    tile_bf16_4x64_eval and tile_bf16_1x32_eval the affine-ReLU lattice kernels igemm_lattice_kernel<4, 1, 4, 1, 2> (and
    igemm_lattice_wide_kernel<2>) on 16 and 4 items, tile_f32_4x48_eval the two fp32 DMA tilings.  REPLAY_NAMED asserts these."""
    c = REPLAY_CONFIGS[config]
    mode = c["mode"]
    calls = distinct_calls(record_step(**c))
    issued = sorted({k[0] for k in calls})
    missing = [s for s in issued if s not in RUNNERS and s not in REPLAY_EXEMPT]
    assert not missing, f"{config}: symbols issued by the step with neither a replay runner nor an exemption: {missing}"
    calls = {k: v for k, v in calls.items() if k[0] in RUNNERS}
    if config in REPLAY_ONLY:
        calls = {k: v for k, v in calls.items() if k[0] in NON_CONV or any(part in k[0] for part in REPLAY_ONLY[config])}
    print(f"\n{config}: {len(calls)} distinct calls, symbols issued: {issued}")
    reached = {}
    for key, (kw, kernel) in sorted(calls.items(), key=lambda kv: str(kv[0])):
        sym = key[0]
        if key in REPLAYED:                        # the same call, already replayed under an earlier config
            reached.setdefault(sym, set()).add("(replayed earlier)")
            continue
        name = RUNNERS[sym](kw)
        REPLAYED.add(key)
        reached.setdefault(sym, set()).add(name or "-")
        if name is not None:                       # (the elementwise / reduction kernels name no matrix-core kernel)
            assert name == kernel, (sym, kw, kernel, name)
        torch.cuda.empty_cache()
    for sym in sorted(reached):
        print(f"  {sym}: {sorted(reached[sym])}")
    for sym in issued:
        assert sym in reached or sym in REPLAY_EXEMPT or config in REPLAY_ONLY, (config, sym)
    if mode == "train":
        assert ("unetdc_adam_step" in issued) == c["adam"], (config, issued)
        # the first layer's weight gradient: BatchNorm backward on load (with its coefficients) where the library supports it
        # (C_in = 1), the plain form after unetdc_bn_relu_bwd otherwise
        first = ("unetdc_conv3x3_first_wgrad_bn", "unetdc_bn_relu_bwd_coeffs") if c["cin"] == 1 else ("unetdc_conv3x3_first_wgrad",)
        for sym in first + ("unetdc_bn_finalize", "unetdc_focal_dice_loss_fwd", "unetdc_focal_dice_loss_bwd", "unetdc_head_fwd_bn",
                            "unetdc_head_bwd_bnstats", "unetdc_bn_relu_bwd", "unetdc_bn_relu_bwd_head"):
            if c["loss"] != "focal" and "focal" in sym:         # combined_loss (train.py) is ATen arithmetic, no loss kernel
                continue
            assert sym in reached, (config, sym, sorted(reached))
    elif mode == "eval":
        assert {"unetdc_bn_eval_affine", "unetdc_head_fwd"} <= set(reached), (config, sorted(reached))
    else:
        assert {"unetdc_bn_frozen_affine", "unetdc_bn_relu_bwd_frozen"} <= set(reached), (config, sorted(reached))
    if config == "dc3_bf16_5x384":
        # the routes the docstring names (no other config has batch 5, so none of these calls was replayed earlier)
        assert "igemm_dma_kernel<__bf16, 4, 2, 2>" in reached["unetdc_convT2x2_fwd"], reached
        assert "wgrad_dma_kernel<__bf16, 4>" in reached["unetdc_convT2x2_wgrad"], reached
        assert "wgrad_dma_kernel<__bf16, 2>" in reached["unetdc_conv3x3_wgrad"], reached
        assert "igemm_dma16_kernel<4, 2, 4> ring3" in reached["unetdc_conv3x3_dgrad_colsum"], reached
    for sym, names in REPLAY_NAMED.get(config, {}).items():
        # the routes the docstring names.  None of these calls shows as "(replayed earlier)" in any order of the configs: the
        # key of distinct_calls carries the batch, the map, the dtype and which optional pointers are given, so the configs
        # that share a batch and a size (crop_bf16_4x32 / crop_f32_4x32: the dtype; crop_bf16_1x32 / tile_bf16_1x32_eval:
        # statistics against the affine-ReLU epilogue) share no 3x3 call.  They do share unetdc_convT2x2_fwd at 1 x 32^2,
        # which is why REPLAY_NAMED names no up-convolution forward there.
        assert set(names) <= reached[sym], (config, sym, reached[sym])
    if c["dx"]:
        assert "unetdc_conv3x3_first_dgrad" in reached, (config, sorted(reached))
