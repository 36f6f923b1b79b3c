"""CPU checks of tests/exact_ref.py (no GPU): the exact references agree with ATen in float64, the fixtures keep the
exactness rule they claim, the bf16 rounding helper is torch's, the guard check catches a stray write in every region,
and the replay's argument table matches include/unetdc_hip.h."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import exact_ref as X
from unet_dc_segmentation_amd._lib import SIGNATURES


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", [(2, 7, 9, 3, 5, 1), (1, 6, 10, 4, 3, 2), (1, 5, 5, 2, 2, 4), (2, 16, 24, 8, 4, 8),
                                  (1, 33, 40, 3, 4, 16), (1, 40, 36, 2, 3, 32), (1, 1, 3, 2, 2, 1)])
def test_conv3x3_reference_matches_autograd(case):
    n, h, w, ci, co, d = case
    g = gen(1)
    x = torch.randn(n, ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(co, generator=g, dtype=torch.float64)
    dy = torch.randn(n, co, h, w, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, b, padding=d, dilation=d)
    gx, gw = torch.autograd.grad(y, (xr, wr), dy)
    torch.testing.assert_close(X.conv3x3_fwd(nhwc(x), wt, d, b), nhwc(y.detach()))
    torch.testing.assert_close(X.conv3x3_dgrad(nhwc(dy), wt, d), nhwc(gx))
    torch.testing.assert_close(X.conv3x3_wgrad(nhwc(x), nhwc(dy), d), gw)
    # an off > 0 view of a wider buffer (concat-style) is just another [N,H,W,C] tensor for the reference
    wide = torch.randn(n, h, w, ci + 6, generator=g, dtype=torch.float64)
    wide[..., 4:4 + ci] = nhwc(x)
    torch.testing.assert_close(X.conv3x3_fwd(wide[..., 4:4 + ci], wt, d, b), nhwc(y.detach()))


@pytest.mark.parametrize("case", [(2, 6, 8, 5, 3, 1), (1, 9, 7, 8, 4, 2), (2, 12, 20, 6, 9, 4), (1, 8, 8, 4, 5, 32)])
def test_onehot_and_separable_references_match_the_gemm_forms(case):
    n, h, w, ci, co, d = case
    g = gen(2)
    x = X.ints((n, h, w, ci), 2, g, lo=1)
    wt, route = X.onehot_conv3x3(co, ci)
    assert int((wt != 0).sum()) == co
    assert torch.equal(X.conv3x3_fwd_onehot(x, route, co, d).double(), X.conv3x3_fwd(x, wt, d))
    dy = X.ints((n, h, w, co), 2, g)
    assert torch.equal(X.conv3x3_dgrad_onehot(dy, route, ci, d).double(), X.conv3x3_dgrad(dy, wt, d))
    a, u = X.ints((n, h, w), 2, g), X.ints((ci,), 2, g)
    assert torch.equal(X.conv3x3_wgrad_separable(a, u, dy, d), X.conv3x3_wgrad(a[..., None] * u, dy, d))
    # the fp32 GEMM form is exact under the rule, and equal to the fp64 one
    assert torch.equal(X.conv3x3_fwd(x, wt, d, fast=True).double(), X.conv3x3_fwd(x, wt, d))


# (n, h, w, ci, co, d): the shapes of tests/test_gpu_exact.py SMALL_ROUTE_CASES at a reduced channel count
PADDED_TAP_CASES = [(1, 2, 2, 24, 16, 16), (3, 3, 3, 24, 16, 16), (2, 8, 8, 24, 16, 4)]


@pytest.mark.parametrize("case", PADDED_TAP_CASES)
def test_references_where_the_dilation_reaches_the_map_side(case):
    """d >= the map side (2 x 2 and 3 x 3 under d = 16): the eight off-centre taps read only padding, so every reference form
    -- GEMM, one-hot, separable -- reduces to the centre tap: forward and input gradient are the 1 x 1 convolution with
    w[:, :, 1, 1], and the eight padded taps of the weight gradient are EXACTLY zero.  At 8 x 8 under d = 4 every tap has a
    4 x 4 (or 4 x 8, 8 x 4) valid rectangle.  All against ATen in float64."""
    n, h, w, ci, co, d = case
    g = gen(8)
    x = torch.randn(n, ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(n, co, h, w, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, padding=d, dilation=d)
    gx, gw = torch.autograd.grad(y, (xr, wr), dy)
    fwd, dg, wg = X.conv3x3_fwd(nhwc(x), wt, d), X.conv3x3_dgrad(nhwc(dy), wt, d), X.conv3x3_wgrad(nhwc(x), nhwc(dy), d)
    torch.testing.assert_close(fwd, nhwc(y.detach()))
    torch.testing.assert_close(dg, nhwc(gx))
    torch.testing.assert_close(wg, gw)
    centre = torch.zeros(3, 3, dtype=torch.bool)
    centre[1, 1] = True
    padded = d >= max(h, w)
    if padded:
        assert bool((wg[:, :, ~centre] == 0).all()) and bool((gw[:, :, ~centre] == 0).all())
        torch.testing.assert_close(fwd, torch.einsum("nhwi,oi->nhwo", nhwc(x), wt[:, :, 1, 1]))
        torch.testing.assert_close(dg, torch.einsum("nhwo,oi->nhwi", nhwc(dy), wt[:, :, 1, 1]))
    else:
        assert bool((wg.abs().amax(dim=(0, 1)) > 0).all())
    # the integer fixtures of the GPU tests: the one-hot and separable forms equal the GEMM forms bit for bit
    xi = X.ints((n, h, w, ci), 2, g, lo=1)
    wo, route = X.onehot_conv3x3(co, ci)
    assert torch.equal(X.conv3x3_fwd_onehot(xi, route, co, d).double(), X.conv3x3_fwd(xi, wo, d))
    dyi = X.ints((n, h, w, co), 2, g)
    assert torch.equal(X.conv3x3_dgrad_onehot(dyi, route, ci, d).double(), X.conv3x3_dgrad(dyi, wo, d))
    a, u = X.ints((n, h, w), 2, g), X.ints((ci,), 2, g)
    sep, dense = X.conv3x3_wgrad_separable(a, u, dyi, d), X.conv3x3_wgrad(xi, dyi, d)
    assert torch.equal(sep, X.conv3x3_wgrad(a[..., None] * u, dyi, d))
    if padded:
        assert bool((sep[:, :, ~centre] == 0).all()) and bool((dense[:, :, ~centre] == 0).all())
        tap_of = route[1]
        off = tap_of != 4                          # output channels routed through a padded tap read nothing
        assert bool(off.any()) and bool((X.conv3x3_fwd_onehot(xi, route, co, d)[..., off] == 0).all())


@pytest.mark.parametrize("case", [(2, 3, 5, 6, 4), (1, 4, 4, 3, 8), (1, 2, 2, 16, 8), (3, 3, 3, 16, 8)])
def test_conv_transpose_reference_matches_autograd(case):
    n, h, w, ci, co = case
    g = gen(3)
    x = torch.randn(n, ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(ci, co, 2, 2, generator=g, dtype=torch.float64)
    b = torch.randn(co, generator=g, dtype=torch.float64)
    dup = torch.randn(n, co, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    up = F.conv_transpose2d(xr, wr, b, stride=2)
    gx, gw = torch.autograd.grad(up, (xr, wr), dup)
    torch.testing.assert_close(X.convT2x2_fwd(nhwc(x), wt, b), nhwc(up.detach()))
    torch.testing.assert_close(X.convT2x2_dgrad(nhwc(dup), wt), nhwc(gx))
    torch.testing.assert_close(X.convT2x2_wgrad(nhwc(x), nhwc(dup)), gw)
    wo = X.onehot_convT2x2(ci, co)
    assert torch.equal((wo != 0).sum(0), torch.ones(co, 2, 2, dtype=torch.long))     # each (co, tap) reads one channel


@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("shape", [(2, 7, 9, 1), (1, 10, 12, 2), (1, 5, 6, 8)])
def test_first_layer_reference_matches_autograd(cin, shape):
    n, h, w, d = shape
    g = gen(4)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(8, cin, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(n, 8, h, w, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, padding=d, dilation=d)
    gx, gw = torch.autograd.grad(y, (xr, wr), dy)
    torch.testing.assert_close(X.first_fwd(x, wt, d), nhwc(y.detach()))
    torch.testing.assert_close(X.first_wgrad(x, nhwc(dy), d), gw)
    torch.testing.assert_close(X.first_dgrad(nhwc(dy), wt, d), gx)


def test_bn_relu_pool_and_column_sums():
    g = gen(5)
    y = torch.randn(2, 6, 8, 5, generator=g, dtype=torch.float64)
    s, t = torch.rand(5, generator=g, dtype=torch.float64) + 0.5, torch.randn(5, generator=g, dtype=torch.float64)
    a = X.bn_relu(y, s, t)
    ref = torch.relu(y * s + t)
    torch.testing.assert_close(a, ref)
    torch.testing.assert_close(X.maxpool2(a), nhwc(F.max_pool2d(ref.permute(0, 3, 1, 2), 2)))
    torch.testing.assert_close(X.colsum(a), ref.sum(dim=(0, 1, 2)))


def test_exactness_rule():
    X.assert_exact(9 * 1024, 2, 2)
    X.assert_exact(4 * 1024 * 1024 - 1, 2, 2)
    with pytest.raises(AssertionError):
        X.assert_exact(4 * 1024 * 1024, 2, 2)
    # weight gradient at 1024^2 bs 4: K = 4.19 M products -> {-1..1}
    assert X.value_range(4 * 1024 * 1024) == 1 and X.value_range(2 * 1024 * 1024) == 2
    with pytest.raises(AssertionError):
        X.value_range(1 << 24)
    # what the GPU fixtures use: dense weights / inputs in {-2..2} for the deepest K of the network (9 * 1024),
    # one-hot inputs positive {1, 2}, and exact sums after a power-of-two BatchNorm scale and an integer shift
    g = gen(6)
    w = X.dense_conv3x3(64, 1024, g)
    assert float(w.abs().max()) <= 2 and bool((w == w.round()).all())
    assert not torch.equal(w, w.flip(2, 3))
    X.assert_exact(9 * 1024, 2 * 2 + 2, w.abs().max())          # relu(2 * x + t), |x| <= 2, t in {-2..2}
    s = X.pow2(64, g, (-1, 0, 1))
    assert bool((torch.log2(s) == torch.log2(s).round()).all())
    ci_of, tap_of, v_of = X.onehot_route(1024, 512)
    assert set(tap_of.tolist()) == set(range(9)) and set(v_of.tolist()) == {1, 2, -1}
    assert set((ci_of // 64).tolist()) == set(range(8))        # every 64-channel block of the input is read


def test_bf16_rounding_helper_is_torchs():
    g = gen(7)
    x = torch.randn(1 << 16, generator=g) * torch.pow(2.0, torch.randint(-30, 30, (1 << 16,), generator=g).float())
    bits = torch.randint(-(1 << 31), (1 << 31) - 1, (1 << 16,), generator=g, dtype=torch.int64).to(torch.int32)
    edge = torch.tensor([0.0, -0.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 257.0, 259.0, 3.4e38, -3.4e38, float("inf"),
                         float("-inf"), 2 ** -130])
    for v in (x, bits.view(torch.float32), edge):
        fin = torch.isfinite(v) | torch.isinf(v)
        assert torch.equal(X.round_bf16(v[fin]).view(torch.int16), v[fin].to(torch.bfloat16).view(torch.int16))
        assert bool(torch.isnan(X.round_bf16(v[~fin]).float()).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("where", ["before", "after", "padding", "left_padding"])
def test_guard_catches_a_single_stray_write(dtype, where):
    c = X.carve(5, 6, 16, 4, dtype, 2, device="cpu")
    c.view.fill_(3.0)
    assert X.guard_violations(c)[1] == 0
    flat = c.buf
    pos = {"before": 2 * 16 - 1, "after": (2 + 5) * 16, "padding": (2 + 3) * 16 + 4 + 6, "left_padding": (2 + 1) * 16 + 3}[where]
    flat[pos] = 0.0
    where_, nbad = X.guard_violations(c)
    assert nbad == 1
    with pytest.raises(AssertionError, match="outside the view"):
        X.assert_guard(c, "stray")
    # a different NaN is a write too: the check compares bits, not values
    flat[pos] = float("nan")
    assert X.guard_violations(c)[1] == (0 if flat.view(X.INT_VIEW[dtype])[pos] == X._signed(X.NAN_BITS[dtype], dtype) else 1)


def test_stats_guard_catches_a_write_past_the_declared_rows():
    declared = (3 + 64) * 2 * 8
    c = X.stats_guard(declared, device="cpu")
    c.view.zero_()
    assert X.guard_violations(c)[1] == 0
    c.buf[declared] = 1.0
    assert X.guard_violations(c) == ([(0, declared)], 1)


def test_input_sentinel_is_finite_after_the_bn_affine():
    for dt in (torch.bfloat16, torch.float32):
        c = X.carve(2, 2, 4, 1, dt, 1, fill="sentinel", device="cpu")
        s = torch.tensor(4.0, dtype=dt)
        assert bool(torch.isfinite(c.buf * s - 2).all())


def test_argument_table_matches_the_header():
    hdr = X.parse_header()
    assert len(hdr) >= len(SIGNATURES) - 1
    for sym, names in X.ARGS.items():
        assert hdr[sym] == names, (sym, hdr[sym], names)
        assert len(SIGNATURES[sym][1]) == len(names), sym
        kinds = X.arg_kinds(SIGNATURES[sym][1])
        pos = X.positions(sym, kinds)
        for key in X.REPLAY_KEYS.get(sym, ("n", "h", "w", "dtype")):
            assert key in pos, (sym, key)
        assert all(names[i].startswith("ld") for k, i in pos.items() if k.startswith("ld"))


# ---------------------------------------------------------------------------------------------------- BatchNorm, head, loss
@pytest.mark.parametrize("rows,count", [(1, 64), (7, 3 * 5 * 7), (600, 1 << 12)])
def test_bn_finalize_reference_matches_batch_norm(rows, count):
    g = gen(11)
    c = 6
    y = torch.randn(count, c, generator=g, dtype=torch.float64) * 2 + 0.5
    cut = torch.sort(torch.randperm(count - 1, generator=g)[: rows - 1] + 1).values.tolist()
    parts = torch.stack([torch.stack([b.sum(0), (b * b).sum(0)]) for b in torch.tensor_split(y, cut)])
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    ref = X.bn_finalize(parts, count, gamma, beta, 1e-5, 0.1, rm, rv)
    rm2, rv2 = rm.clone(), rv.clone()
    out = F.batch_norm(y, rm2, rv2, gamma, beta, training=True, momentum=0.1, eps=1e-5)
    torch.testing.assert_close(ref["running_mean"], rm2)
    torch.testing.assert_close(ref["running_var"], rv2)
    torch.testing.assert_close(y * ref["scale"] + ref["shift"], out)
    torch.testing.assert_close(ref["mean"], y.mean(0))
    fr = X.bn_frozen_affine(gamma, beta, rm, rv, 1e-5)
    torch.testing.assert_close(y * fr["scale"] + fr["shift"], F.batch_norm(y, rm, rv, gamma, beta, training=False, eps=1e-5))
    bias = torch.randn(c, generator=g, dtype=torch.float64)
    ev = X.bn_eval_affine(gamma, beta, rm, rv, 1e-5, bias)
    torch.testing.assert_close(y * ev["scale"] + ev["shift"], F.batch_norm(y + bias, rm, rv, gamma, beta, training=False, eps=1e-5))


def test_bn_finalize_fixture_is_exact_at_any_count():
    """tests/test_gpu_exact_norm.py finalize_parts at the counts of its off-grid cases: the kernel's own double arithmetic
    (total / count, total_q / count - mean^2, 1 / sqrt, one rounding to fp32, the fp32 products of scale and shift) lands on
    the fp32 rounding of the fp64 reference exactly, so those cases keep bound 0 for mean, var, rstd, scale and shift."""
    from tests import test_gpu_exact_norm as N
    assert any(not N.pow2_count(count) for _, count, _ in N.ODD_FINALIZE_CASES)
    for rows, count, c in N.FINALIZE_CASES + N.ODD_FINALIZE_CASES + N.SMALL_FINALIZE_CASES:
        if rows * c > 1 << 20:                   # (the largest power-of-two cases: minutes of host time for nothing new)
            continue
        g = gen(31)
        parts, m, var = N.finalize_parts(rows, count, c, g, dev="cpu")
        gamma = X.pow2(c, g, (-1, 0, 1)) * (1 - 2 * (torch.rand(c, generator=g) < 0.3).float())
        beta = X.ints((c,), 3, g)
        ref = X.bn_finalize(parts.double(), count, gamma, beta, 0.0, 0.1)
        # the kernel, statement by statement (bn_finalize_kernel): fp32 rows summed in double, any order (integers: exact)
        s, q = parts[:, 0].double().flip(0).sum(0), parts[:, 1].double().flip(0).sum(0)
        mean = s / float(count)
        v = (q / float(count) - mean * mean).clamp_min(0.0)
        rstd = (1.0 / torch.sqrt(v)).float()
        sc = gamma * rstd
        sh = beta - mean.float() * sc
        assert torch.equal(mean, m) and torch.equal(v, var), (rows, count, c)
        for got, k in ((mean.float(), "mean"), (rstd, "rstd"), (sc, "scale"), (sh, "shift")):
            assert not X.within_bound(got, ref[k], 0, torch.float32).any(), (rows, count, c, k)
        if rows > 2 and rows == -(-count // 256) and count % 256:      # one row per 256-pixel block: the last one is partial
            assert float(parts[-1, 1].abs().max()) < float(parts[1, 1].abs().max()), (rows, count)


@pytest.mark.parametrize("count", [45, 120, 4, 3 << 18, 4800, 5 * 384 * 384, 1 << 12])
def test_bn_bwd_coefficient_bounds_hold_the_kernels_double_arithmetic(count):
    """exact_ref.bn_bwd_coeff_bounds: the kernel's double evaluation, in its own association (a S / M, a = gamma rstd) and in
    another one (a (S / M)), rounded to fp32 once, lies within the bound of the reference for integer sums and power-of-two
    k1; an fp32 division by a count rounded up to a multiple of 256 does not; at a power-of-two count the bound is not needed
    (equality)."""
    g = gen(41)
    c = 512
    s1, s2, s3 = (X.ints((c,), 4000, g).double() for _ in range(3))
    gamma, rs = (X.pow2(c, g, (-1, 0, 1)) * (1 - 2 * (torch.rand(c, generator=g) < 0.3).float())).double(), X.pow2(c, g, (-1, 0)).double()
    k1 = gamma * rs
    k2, k3 = k1 * s1 / count, k1 * s2 / count
    dbias = -k3 * s3
    b = X.bn_bwd_coeff_bounds(k2, k3, dbias)
    for assoc in (lambda s: k1 * s / float(count), lambda s: k1 * (s / float(count))):
        for got, ref, bnd in ((assoc(s1), k2, "k2_bound"), (assoc(s2), k3, "k3_bound"), (-assoc(s2) * s3, dbias, "dbias_bound")):
            zero = torch.zeros_like(ref) if count & (count - 1) == 0 else b[bnd]
            assert not X.within_bound(got.float(), ref, zero, torch.float32).any(), (count, bnd)
    if count % 256:
        wrong = k1 * s1 / float(-(-count // 256) * 256)
        assert X.within_bound(wrong.float(), k2, b["k2_bound"], torch.float32)[s1 != 0].all()


def _bn_autograd(y, gamma, beta, rm, rv, dskip, dpool, frozen):
    """dL/dy, dL/dgamma, dL/dbeta, dL/dbias (bias added to the conv output in front of the BatchNorm) by autograd, NCHW."""
    yr, gr, br = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = torch.relu(F.batch_norm(yr, rm.clone(), rv.clone(), gr, br, training=not frozen, momentum=0.1, eps=1e-5))
    out = (a * dskip).sum() if dskip is not None else 0
    if dpool is not None:
        out = out + (F.max_pool2d(a, 2) * dpool).sum()
    gy, gg, gb = torch.autograd.grad(out, (yr, gr, br))
    return gy, gg, gb, gy.sum(dim=(0, 2, 3))


@pytest.mark.parametrize("form", ["skip", "pool", "skip+pool", "frozen", "frozen+pool"])
def test_bn_relu_backward_reference_matches_autograd(form):
    g = gen(12)
    n, c, h, w = 2, 5, 6, 8
    y = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64) * 0.3
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64) * 0.2, torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    dskip = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) if "skip" in form or form == "frozen" else None
    dpool = torch.randn(n, c, h // 2, w // 2, generator=g, dtype=torch.float64) if "pool" in form else None
    frozen = form.startswith("frozen")
    if frozen:
        st = X.bn_frozen_affine(gamma, beta, rm, rv, 1e-5)
        mean, rstd = st["mean"], st["rstd"]
    else:
        mean = y.mean(dim=(0, 2, 3))
        rstd = 1 / torch.sqrt(y.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
        st = dict(scale=gamma * rstd, shift=beta - mean * gamma * rstd)
    ref = X.bn_relu_bwd(nhwc(y), st["scale"], st["shift"], mean, rstd, gamma, None if dskip is None else nhwc(dskip),
                        None if dpool is None else nhwc(dpool), torch.float64, frozen=frozen)
    gy, gg, gb, gbias = _bn_autograd(y, gamma, beta, rm, rv, dskip, dpool, frozen)
    torch.testing.assert_close(ref["dy"], nhwc(gy))
    torch.testing.assert_close(ref["dgamma"], gg)
    torch.testing.assert_close(ref["dbeta"], gb)
    torch.testing.assert_close(ref["dbias"], gbias, atol=1e-12, rtol=1e-9)


def test_pool_argmax_is_atens_first_maximum():
    """Windows full of ties (and ReLU zeros): the reference routes the pooled gradient like ATen's max_pool2d backward."""
    g = gen(13)
    a = torch.relu(X.ints((2, 3, 8, 10), 1, g).double())          # {0, 1}: almost every window has a tie
    dpool = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    ar = a.clone().requires_grad_(True)
    ga, = torch.autograd.grad((F.max_pool2d(ar, 2) * dpool).sum(), ar)
    mine = X.pool_scatter(nhwc(dpool), X.pool_argmax(nhwc(a)), 8, 10)
    assert torch.equal(mine, nhwc(ga))
    assert int((X.pool_argmax(nhwc(a)) == 0).sum()) > 0 and int((X.pool_argmax(nhwc(a)) == 3).sum()) > 0


@pytest.mark.parametrize("oc", [1, 2])
def test_head_reference_matches_autograd(oc):
    g = gen(14)
    n, c, h, w = 2, 16, 5, 7
    a = torch.relu(torch.randn(n, c, h, w, generator=g, dtype=torch.float64))
    wt, b = torch.randn(oc, c, generator=g, dtype=torch.float64), torch.randn(oc, generator=g, dtype=torch.float64)
    dprobs = torch.randn(n, oc, h, w, generator=g, dtype=torch.float64)
    ar, wr, br = a.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    probs = torch.sigmoid(F.conv2d(ar, wr[:, :, None, None], br))
    ga, gw, gb = torch.autograd.grad(probs, (ar, wr, br), dprobs)
    am = nhwc(a).reshape(-1, c)
    _, p = X.head_fwd(am, wt, b, n, h, w)
    torch.testing.assert_close(p, probs.detach())
    ref = X.head_bwd(dprobs, p, am, wt, torch.float64)
    torch.testing.assert_close(ref["dw"], gw)
    torch.testing.assert_close(ref["db"], gb)
    torch.testing.assert_close(ref["da"], nhwc(ga).reshape(-1, c))
    # the fused BatchNorm-backward sums are bn_relu_bwd's sums with dskip = da
    y = torch.randn(n * h * w, c, generator=g, dtype=torch.float64)
    sc, sh, mu, rs = (torch.randn(c, generator=g, dtype=torch.float64) for _ in range(4))
    ref = X.head_bwd(dprobs, p, am, wt, torch.float64, bn=(y, sc, sh, mu, rs))
    bn = X.bn_relu_bwd(y.view(n, h, w, c), sc, sh, mu, rs, torch.ones(c, dtype=torch.float64), ref["da"].view(n, h, w, c),
                       None, torch.float64)
    for k in ("s1", "s2", "s3"):
        torch.testing.assert_close(ref[k], bn[k])


@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_focal_dice_reference_matches_autograd(gamma):
    from utils.metrics_DC import focal_dice_loss
    g = gen(15)
    n, h, w = 3, 6, 9
    p = torch.rand(n, 1, h, w, generator=g, dtype=torch.float64) * 0.98 + 0.01
    t = (torch.rand(n, 1, h, w, generator=g, dtype=torch.float64) < 0.3).double()
    t[0, 0, 0, :3] = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)       # soft targets too
    pr = p.clone().requires_grad_(True)
    loss = focal_dice_loss(pr, t, alpha=0.8, gamma=gamma, ratio=0.3)
    gp, = torch.autograd.grad(loss, pr)
    ref = X.focal_dice(p.view(n, -1), t.view(n, -1), 0.8, gamma, 0.3, 1e-7)
    torch.testing.assert_close(ref["loss"], loss.detach())
    torch.testing.assert_close(ref["dp"], gp.view(n, -1))


def _loss_fp32(p, t, alpha, gamma, ratio, smooth, gout):
    """csrc/loss.hip restated in fp32 torch arithmetic (sums in fp32 over one chain per map)."""
    f32 = torch.float32
    lp, lq = torch.log(p), torch.log1p(-p)
    bce = -(t * lp.clamp_min(-100) + (1 - t) * lq.clamp_min(-100))
    dbce = -(torch.where(lp > -100, t / p, torch.zeros_like(p)) - torch.where(lq > -100, (1 - t) / (1 - p), torch.zeros_like(p)))
    pt = torch.exp(-bce)
    om = 1 - pt
    omg1 = om if gamma == 2.0 else torch.pow(om, torch.tensor(gamma - 1, dtype=f32))
    omg = omg1 * om
    focal = alpha * omg * bce
    dfocal = alpha * (gamma * omg1 * pt * bce + omg) * dbce
    nimg, hw = p.shape
    sums = [torch.cumsum(x, 1, dtype=f32)[:, -1].double() for x in (focal, p * t, p, t)]
    u = sums[2] + sums[3] + float(smooth)
    dice = (2 * sums[1] + float(smooth)) / u
    loss = (ratio * (float(sums[0].sum()) / (nimg * hw)) + (1 - ratio) * (1 - float(dice.sum()) / nimg))
    c1, c2 = (2 / u).float(), ((2 * sums[1] + float(smooth)) / (u * u)).float()
    kf = torch.tensor(ratio / (nimg * hw), dtype=torch.float64).float()
    kd = (1 - torch.tensor(ratio, dtype=f32)) / torch.tensor(float(nimg))
    dp = gout * (kf * dfocal - kd * (t * c1[:, None] - c2[:, None]))
    return torch.tensor(loss).float(), dp


@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_focal_dice_bounds_hold_an_fp32_evaluation(gamma):
    """The interval bounds the GPU tests use contain an fp32 evaluation of the same formula, at the edge values they test
    (p of 0, 1, 1e-45 and 1 - 2^-24, i.e. the log clamp), and stay tight on ordinary values."""
    g = gen(16)
    nimg, hw = 3, 4096
    p = torch.rand(nimg, hw, generator=g)
    p[:, :8] = torch.tensor([0.0, 1.0, 1e-45, 1 - 2 ** -24] * 2)
    t = (torch.rand(nimg, hw, generator=g) < 0.2).float()
    t[:, :8] = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    alpha, ratio, smooth, gout = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.8, 0.3, 1e-7, -1.75))
    loss, dp = _loss_fp32(p, t, alpha, gamma, ratio, smooth, gout)
    (llo, lhi), (dlo, dhi) = X.focal_dice_bounds(p, t, alpha, gamma, ratio, smooth, gout, nsum=hw + 8)
    assert float(llo) <= float(loss) <= float(lhi)
    dpd = dp.double()
    assert bool(((dpd >= dlo) & (dpd <= dhi)).all())
    ref = X.focal_dice(p, t, alpha, gamma, ratio, smooth)
    assert float(lhi - llo) < 4 * (hw + 8) * X.EPS32 * abs(float(ref["loss"]))       # the summation term dominates
    width = (dhi - dlo)[:, 8:]
    assert float((width / (gout * ref["dp"][:, 8:]).abs()).max()) < 1e-2         # (nsum = hw here: the GPU sums are far shorter)


# ---------------------------------------------------------------------------------------------------- optimizer
def _adam_fixture(n, g):
    """Parameters, signed first moments, non-negative second moments and gradients spanning many decades, with exact zeros."""
    p = torch.randn(n, generator=g) * 0.05
    mag = lambda lo, hi: torch.exp(torch.empty(n).uniform_(lo, hi, generator=g))     # noqa: E731
    grad = torch.randn(n, generator=g).sign() * mag(-30.0, 6.0)
    m = torch.randn(n, generator=g).sign() * mag(-25.0, 2.0)
    v = mag(-40.0, 4.0)
    grad[::7], m[::11], v[::13] = 0.0, 0.0, 0.0
    return p, m, v, grad


@pytest.mark.parametrize("step", [1, 2, 10000])
@pytest.mark.parametrize("hyper", [(1e-3, 0.9, 0.999, 1e-8, 1.0), (3e-4, 0.8, 0.95, 1e-6, 1 / 3)])
def test_adam_reference_matches_torch_adam(step, hyper):
    """exact_ref.adam_step is torch.optim.Adam's step (fp64, CPU) from a given state; grad_scale multiplies the gradient."""
    lr, b1, b2, eps, gs = hyper
    p, m, v, grad = (t.double() for t in _adam_fixture(4096, gen(20)))
    w = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(step - 1), dtype=torch.float64), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    w.grad = grad * gs
    opt.step()
    rp, rm, rv = X.adam_step(p, m, v, grad, step, lr, b1, b2, eps, gs)
    torch.testing.assert_close(rm, opt.state[w]["exp_avg"], rtol=1e-13, atol=0)
    torch.testing.assert_close(rv, opt.state[w]["exp_avg_sq"], rtol=1e-13, atol=0)
    torch.testing.assert_close(rp, w.detach(), rtol=1e-13, atol=1e-300)


def _fma32(a, b, c):
    """fmaf in fp64 arithmetic: a * b is exact in fp64, the sum rounds once more before the fp32 rounding (never an issue
    at the bound's slack)."""
    return (a.double() * b.double() + c.double()).float()


def _adam_fp32(p, m, v, g, step, lr, b1, b2, eps, gs, bc_step=None):
    """csrc/optim.hip adam_update restated in fp32 torch arithmetic (constants formed in double, rounded once)."""
    f = lambda x: torch.tensor(x, dtype=torch.float64).float()           # noqa: E731
    s = step if bc_step is None else bc_step
    bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
    g = g * f(gs)
    m = _fma32(f(1.0 - b1), g - m, m)
    v = _fma32(v, f(b2), f(1.0 - b2) * g * g)
    den = torch.sqrt(v) * f(1.0 / math.sqrt(bc2)) + f(eps)
    return p - f(lr / bc1) * (m / den), m, v


@pytest.mark.parametrize("step", [1, 2, 12345])
@pytest.mark.parametrize("hyper", [(1e-3, 0.9, 0.999, 1e-8, 1.0), (3e-4, 0.8, 0.95, 1e-6, 1 / 3)])
def test_adam_bounds_hold_an_fp32_evaluation(step, hyper):
    """The per-element bounds the GPU test uses contain an fp32 evaluation of adam_update, are a few ulp wide, and exclude
    the same step with the bias corrections of step - 1 (at the small step counts where that differs)."""
    lr, b1, b2, eps, gs = hyper
    p, m, v, grad = _adam_fixture(1 << 15, gen(21))
    got = _adam_fp32(p, m, v, grad, step, lr, b1, b2, eps, gs)
    ref = X.adam_step(p, m, v, grad, step, lr, b1, b2, eps, gs)
    bounds = X.adam_bounds(p, m, v, grad, step, lr, b1, b2, eps, gs)
    # the scale of each output's terms: the update for p, the moment and the scaled gradient for m (they may cancel), v itself
    scales = ((p.double() - ref[0]).abs() + p.double().abs(), m.double().abs() + (grad.double() * gs).abs(), ref[2])
    for name, gt, r, b, sc in zip("pmv", got, ref, bounds, scales):
        assert not bool(X.within_bound(gt, r, b, torch.float32).any()), name
        assert float((b / (X.EPS32 * sc + 2.0 ** -126)).max()) < 32, name       # a few ulp of the terms, nowhere wider
    assert bool(X.within_bound(torch.zeros(1), torch.ones(1), torch.zeros(1), torch.float32).all())
    if step <= 2:
        wrong = _adam_fp32(p, m, v, grad, step, lr, b1, b2, eps, gs, bc_step=step + 1)
        assert bool(X.within_bound(wrong[0], ref[0], bounds[0], torch.float32).any())
    if gs != 1.0:
        wrong = _adam_fp32(p, m, v, grad, step, lr, b1, b2, eps, 1.0)
        assert float(X.within_bound(wrong[1], ref[1], bounds[1], torch.float32).double().mean()) > 0.5


@pytest.mark.parametrize("case", [(2, 6, 7, 5, 3, 1), (1, 9, 8, 4, 6, 2), (1, 12, 10, 3, 4, 4)])
def test_packed_conv3x3_images_are_the_gemm_operands(case):
    """exact_ref.pack_conv3x3 (the host form of engine.PackedWeights' 3x3 images): nine shifted GEMMs against w_fwd are
    F.conv2d, and against w_dgrad the input gradient."""
    n, h, w, ci, co, d = case
    g = gen(22)
    x = torch.randn(n, ci, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(n, co, h, w, generator=g, dtype=torch.float64)
    y = F.conv2d(x, wt, padding=d, dilation=d)
    gx, = torch.autograd.grad(y, x, dy)
    wf, wd = X.pack_conv3x3(wt)
    assert wf.shape == (9, co, ci) and wd.shape == (9, ci, co)
    torch.testing.assert_close(X.conv3x3_packed(nhwc(x.detach()), wf, d), nhwc(y.detach()))
    torch.testing.assert_close(X.conv3x3_packed(nhwc(dy), wd, d), nhwc(gx))


@pytest.mark.parametrize("case", [(2, 3, 5, 6, 4), (1, 4, 4, 3, 8)])
def test_packed_conv_transpose_images_are_the_gemm_operands(case):
    """exact_ref.pack_convT2x2: w_fwd ([4*Cout][Cin]) gives F.conv_transpose2d, w_dgrad ([4][Cin][Cout]) its input gradient."""
    n, h, w, ci, co = case
    g = gen(23)
    x = torch.randn(n, ci, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(ci, co, 2, 2, generator=g, dtype=torch.float64)
    dup = torch.randn(n, co, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    up = F.conv_transpose2d(x, wt, stride=2)
    gx, = torch.autograd.grad(up, x, dup)
    wf, wd = X.pack_convT2x2(wt)
    assert wf.shape == (4, co, ci) and wd.shape == (4, ci, co)
    torch.testing.assert_close(X.convT2x2_packed(nhwc(x.detach()), wf), nhwc(up.detach()))
    torch.testing.assert_close(X.convT2x2_packed_adj(nhwc(dup), wd), nhwc(gx))
