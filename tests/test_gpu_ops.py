"""GPU parity tests, one per C-ABI operator: HIP kernel vs a plain PyTorch-CPU fp32 evaluation of
the same op (the ATen ops the reference itself calls) on seeded inputs.

Tolerances: fp32 path -- exact-fp32 MFMA, only the summation order differs: rel-L2 <= 2e-5.
bf16 path -- inputs are pre-rounded to bf16 so both sides see identical operands; the error
left is fp32-accumulate order + one bf16 rounding of the output (2^-9): rel-L2 <= 6e-3.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import gpu_ops as G
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd._lib import call

TOL = {"f32": 2e-5, "bf16": 6e-3}
TOL_W = {"f32": 5e-5, "bf16": 8e-3}        # reductions over many pixels


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def gen(seed):
    return torch.Generator().manual_seed(seed)


CONV_CASES = [  # n, h, w, cin, cout, d
    (2, 16, 24, 64, 64, 1),      # narrow tile, ragged M (768 = 3 x 256)
    (1, 16, 24, 64, 64, 2),      # M = 384: ragged last block
    (1, 32, 32, 128, 128, 4),    # wide tile
    (2, 32, 32, 64, 128, 16),    # d = 16 on a 32x32 map: tap skipping
    (1, 16, 16, 256, 64, 8),     # deep K, narrow N
    (1, 8, 8, 128, 256, 1),      # tiny map
    (2, 48, 80, 64, 128, 2),     # map sizes that are not powers of two: division-based pixel decode everywhere
    (3, 96, 160, 64, 64, 1),     # ... 46080 pixels = 180 block tiles; W = 160: five 32-pixel wgrad segments in fp32, per-tap kernel in bf16
    # >= 128K pixels, Cout 64/128, d <= 2: routed to the halo-patch kernel (igemm_halo.hip)
    (2, 256, 256, 64, 64, 1),    # 4-wave config, one K chunk, image borders on all sides
    (1, 264, 512, 128, 64, 1),   # two K chunks through a single patch buffer; H not a power of two
    (2, 256, 256, 64, 128, 2),   # 8-wave config, d = 2
    (1, 512, 256, 128, 128, 2),  # 8-wave config, two K chunks, double-buffered patch
    # bf16: persistent lattice-halo kernel (igemm_lattice.hip) -- several items per workgroup, n-blocks, dilation as lattice stride
    (3, 512, 256, 64, 64, 1),    # 1536 tiles on 512 workgroups: three items each through ONE patch buffer
    (4, 128, 128, 128, 256, 1),  # BN = 128, two n-blocks (constants reloaded per item), two K chunks, two items per workgroup
    (2, 128, 128, 256, 128, 4),  # d = 4: sixteen 32 x 32 sub-lattices per image, four K chunks
    (1, 64, 256, 64, 64, 2),     # d = 2 with the 4-wave configuration, fewer items than workgroups
    (1, 1024, 64, 64, 128, 1),   # tall narrow map: two tiles per row
    # bf16: 16 x 16 pixel blocks as M tiles for d % 16 == 0 (igemm_dma16.hip, block order): every padded tap is skipped
    (3, 48, 80, 128, 64, 16),    # 3 x 5 blocks per image, division-based block decode; border / inner blocks run 4 / 6 / 9 taps
    (1, 64, 64, 64, 128, 32),    # d = 32 on a 64 x 64 map: a tap moves a block by two blocks
]

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv3x3_fwd_dgrad_wgrad(dtype, case):
    n, h, w, cin, cout, d = case
    g = gen(1)
    x = G.quant(torch.randn(n, cin, h, w, generator=g), dtype)
    wt = G.quant(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5), dtype)
    b = torch.randn(cout, generator=g)
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, b, padding=d, dilation=d)
    gx_ref, gw_ref = torch.autograd.grad(y_ref, (xr, wr), dy)

    wf, wd = G.pack_conv(wt, dtype)
    xv = G.to_nhwc(x, dtype, ld=cin + 64, off=64)            # strided input view (concat-style)
    yv = G.empty_nhwc(n * h * w, cout, dtype, ld=2 * cout, off=cout)
    bd = b.cuda()
    st, rows = G.conv3x3_fwd(xv, wf, bd, n, h, w, cin, cout, d, dtype, yv, stats=True)
    y = G.from_nhwc(yv, n, h, w)
    assert rel(y, y_ref.detach()) < TOL[dtype], ("fwd", rel(y, y_ref.detach()))
    # statistics partials: sums of the stored values
    stc = st.cpu()[: rows * 2 * cout].reshape(rows, 2, cout).double().sum(0)
    yq = y.double()
    np.testing.assert_allclose(stc[0].numpy(), yq.sum(dim=(0, 2, 3)).numpy(), rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(stc[1].numpy(), (yq * yq).sum(dim=(0, 2, 3)).numpy(), rtol=1e-4, atol=1e-2)
    # rows that carry data (the persistent kernel writes one row per workgroup and zeros into the rest of the bound)
    live = G.LIVE_ROWS.value
    if dtype == "bf16" and d % 16 == 0 and h % 16 == 0 and w % 16 == 0:
        assert _lib.load().unetdc_last_kernel().decode().endswith("blocks16x16")        # routed to the block-order form
    assert 1 <= live <= rows
    sta = st.cpu()[: rows * 2 * cout].reshape(rows, 2, cout)
    assert torch.equal(sta[live:], torch.zeros_like(sta[live:]))
    assert torch.equal(sta[:live].double().sum(0), stc)
    # run-to-run: same output and same partial rows, bit for bit (fixed tile order per workgroup, fixed reduction trees)
    yv2 = G.empty_nhwc(n * h * w, cout, dtype, ld=2 * cout, off=cout)
    st2, _ = G.conv3x3_fwd(xv, wf, bd, n, h, w, cin, cout, d, dtype, yv2, stats=True)
    assert torch.equal(yv, yv2) and torch.equal(st[: rows * 2 * cout], st2[: rows * 2 * cout])
    # eval-mode epilogue: relu(acc*scale + shift)
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    y2v = G.empty_nhwc(n * h * w, cout, dtype)
    G.conv3x3_fwd(xv, wf, None, n, h, w, cin, cout, d, dtype, y2v, scale=sc.cuda(), shift=sh.cuda())
    y2_ref = torch.relu(F.conv2d(x, wt, None, padding=d, dilation=d) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    assert rel(G.from_nhwc(y2v, n, h, w), y2_ref) < TOL[dtype]
    # dgrad
    dyv = G.to_nhwc(dy, dtype)
    dxv = G.empty_nhwc(n * h * w, cin, dtype, ld=cin + 32)
    G.conv3x3_dgrad(dyv, wd, dxv, n, h, w, cin, cout, d, dtype)
    assert rel(G.from_nhwc(dxv, n, h, w), gx_ref) < TOL[dtype], "dgrad"
    # wgrad
    dw = G.conv3x3_wgrad(xv, dyv, n, h, w, cin, cout, d, dtype).cpu()
    assert rel(dw, gw_ref) < TOL_W[dtype], ("wgrad", rel(dw, gw_ref))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 512, 256, 64, 64, 1), (1, 520, 512, 128, 64, 1), (4, 256, 256, 64, 128, 2),
                                  (2, 128, 128, 256, 128, 8), (8, 64, 64, 128, 256, 4),
                                  (5, 64, 64, 1024, 512, 1)])   # 128 channel tiles x 5 images: two images per workgroup (2 + 2 + 1)
def test_wgrad_tap_fused(dtype, case):
    """>= 256K pixels with a 64-channel side: routed to wgrad_fused.hip (one staging for all 9 taps)."""
    n, h, w, cin, cout, d = case
    g = gen(4)
    x = G.quant(torch.randn(n, cin, h, w, generator=g), dtype)
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    wr = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    gw_ref, = torch.autograd.grad(F.conv2d(x, wr, None, padding=d, dilation=d), wr, dy)
    xv = G.to_nhwc(x, dtype, ld=cin + 64, off=64)
    dw = G.conv3x3_wgrad(xv, G.to_nhwc(dy, dtype), n, h, w, cin, cout, d, dtype).cpu()
    assert rel(dw, gw_ref) < TOL_W[dtype], rel(dw, gw_ref)


@pytest.mark.parametrize("case", [(2, 32, 32, 256, 256, 16), (1, 16, 24, 256, 512, 8), (3, 24, 40, 512, 256, 16),
                                  (8, 32, 32, 512, 1024, 16)])
def test_wgrad_valid_rectangles(case):
    """Strongly dilated layers (the bottleneck: d = 16 on 32 x 32) in bf16: routed to wgrad_rect.hip, where every tap sums
    over its valid output rectangle only and K is cut into equal units (centre tap 4, edge taps 2, corner taps 1 for the
    square case; ragged rectangles and a unit that does not divide the lists in the other cases)."""
    n, h, w, cin, cout, d = case
    g = gen(6)
    x = G.quant(torch.randn(n, cin, h, w, generator=g), "bf16")
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), "bf16")
    wr = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    gw_ref, = torch.autograd.grad(F.conv2d(x, wr, None, padding=d, dilation=d), wr, dy)
    xv = G.to_nhwc(x, "bf16", ld=cin + 64, off=64)
    dw = G.conv3x3_wgrad(xv, G.to_nhwc(dy, "bf16"), n, h, w, cin, cout, d, "bf16")
    assert _lib.load().unetdc_last_kernel().decode().startswith("wgrad_rect_kernel")
    assert rel(dw.cpu(), gw_ref) < TOL_W["bf16"], rel(dw.cpu(), gw_ref)
    dw2 = G.conv3x3_wgrad(xv, G.to_nhwc(dy, "bf16"), n, h, w, cin, cout, d, "bf16")
    assert torch.equal(dw, dw2)                            # fixed summation order: bitwise reproducible


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_wgrad_many_pixels_ksplit(dtype):
    """K (pixels) large enough that several K-slices and a ragged last slice are exercised."""
    n, h, w, cin, cout, d = 2, 96, 80, 64, 64, 2
    g = gen(3)
    x = G.quant(torch.randn(n, cin, h, w, generator=g), dtype)
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    wr = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    gw_ref, = torch.autograd.grad(F.conv2d(x, wr, None, padding=d, dilation=d), wr, dy)
    dw = G.conv3x3_wgrad(G.to_nhwc(x, dtype), G.to_nhwc(dy, dtype), n, h, w, cin, cout, d, dtype).cpu()
    assert rel(dw, gw_ref) < TOL_W[dtype], rel(dw, gw_ref)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("shape", [(2, 24, 40, 1), (2, 64, 64, 2), (3, 10, 10, 1), (1, 8, 8, 1), (2, 96, 136, 1)])
def test_first_conv(dtype, cin, shape):
    """(2,24,40): fp32-MFMA kernels, division path; (2,64,64) d=2: shift path, several workgroups; W % 8 == 0 with d = 1 and
    C_in = 1: the row-run weight-gradient kernel (one run per row at 8 x 8: both edges in one run; 96 x 136: several trips);
    (3,10,10): pixel count not a multiple of 32 -> VALU kernels of first_conv.hip."""
    n, h, w, d = shape
    cout = 64
    g = gen(5)
    x = torch.rand(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / 3
    b = torch.randn(cout, generator=g)
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    wr = wt.clone().requires_grad_(True)
    y_ref = F.conv2d(x, wr, b, padding=d, dilation=d)
    gw_ref, = torch.autograd.grad(y_ref, wr, dy)
    xd, wdv, bd = x.cuda(), wt.cuda(), b.cuda()
    rows = _lib.load().unetdc_conv3x3_first_stats_rows(n * h * w, cin, cout)
    st = torch.full(((rows + 64) * 2 * cout,), float("nan"), device="cuda")
    yv = G.empty_nhwc(n * h * w, cout, dtype)
    call("unetdc_conv3x3_first_fwd", xd.data_ptr(), wdv.data_ptr(), bd.data_ptr(), None, None, yv.data_ptr(),
         yv.stride(0), st.data_ptr(), n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    y = G.from_nhwc(yv, n, h, w)
    assert rel(y, y_ref.detach()) < (2e-6 if dtype == "f32" else 4e-3)
    stc = st.cpu()[: rows * 2 * cout].reshape(rows, 2, cout).double().sum(0)
    np.testing.assert_allclose(stc[0].numpy(), y.double().sum(dim=(0, 2, 3)).numpy(), rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(stc[1].numpy(), (y.double() ** 2).sum(dim=(0, 2, 3)).numpy(), rtol=1e-4, atol=1e-2)
    # eval epilogue
    sc, sh = (torch.rand(cout, generator=g) + 0.5), torch.randn(cout, generator=g)
    scd, shd = sc.cuda(), sh.cuda()          # keep the device tensors alive across the call
    y2v = G.empty_nhwc(n * h * w, cout, dtype)
    call("unetdc_conv3x3_first_fwd", xd.data_ptr(), wdv.data_ptr(), None, scd.data_ptr(), shd.data_ptr(),
         y2v.data_ptr(), y2v.stride(0), None, n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    y2_ref = torch.relu(F.conv2d(x, wt, None, padding=d, dilation=d) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    assert rel(G.from_nhwc(y2v, n, h, w), y2_ref) < (2e-6 if dtype == "f32" else 4e-3)
    # wgrad
    nbytes = _lib.load().unetdc_conv3x3_first_wgrad_workspace(n, h, w, cin, cout)
    ws = G.workspace(nbytes)
    dyv = G.to_nhwc(dy, dtype)
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    call("unetdc_conv3x3_first_wgrad", xd.data_ptr(), dyv.data_ptr(), dyv.stride(0), dw.data_ptr(), ws.data_ptr(),
         nbytes, n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    assert rel(dw.cpu(), gw_ref) < 2e-5


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 8, 12, 128, 64), (1, 16, 16, 256, 128), (1, 4, 4, 1024, 512),
                                  # W % 32 == 0: the tap-fused weight gradient (convt_wgrad.hip, bf16): one / several channel tiles,
                                  # several K slices, rows of 32 / 64 / 96 pixels, two images
                                  (2, 32, 32, 256, 128), (1, 64, 64, 128, 64), (2, 16, 96, 512, 256), (1, 32, 32, 1024, 512),
                                  # the shortest K range the plan accepts (two 32-pixel steps per half); a half that crosses an image
                                  (1, 4, 32, 128, 64), (3, 8, 32, 128, 64)])
def test_conv_transpose(dtype, case):
    n, h, w, cin, cout = case
    g = gen(7)
    x = G.quant(torch.randn(n, cin, h, w, generator=g), dtype)
    wt = G.quant(torch.randn(cin, cout, 2, 2, generator=g) / cin ** 0.5, dtype)
    b = torch.randn(cout, generator=g)
    dup = G.quant(torch.randn(n, cout, 2 * h, 2 * w, generator=g), dtype)
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y_ref = F.conv_transpose2d(xr, wr, br, stride=2)
    gx_ref, gw_ref, gb_ref = torch.autograd.grad(y_ref, (xr, wr, br), dup)
    wf, wd = G.pack_convT(wt, dtype)
    xv = G.to_nhwc(x, dtype)
    upv = G.empty_nhwc(n * 4 * h * w, cout, dtype, ld=2 * cout, off=0)       # first half of a concat buffer
    bdev = b.cuda()
    call("unetdc_convT2x2_fwd", xv.data_ptr(), xv.stride(0), wf.data_ptr(), bdev.data_ptr(), upv.data_ptr(),
         upv.stride(0), n, h, w, cin, cout, G.DT[dtype], G.stream())
    assert rel(G.from_nhwc(upv, n, 2 * h, 2 * w), y_ref.detach()) < TOL[dtype]
    dupv = G.to_nhwc(dup, dtype, ld=2 * cout, off=0)
    dxv = G.empty_nhwc(n * h * w, cin, dtype)
    call("unetdc_convT2x2_dgrad", dupv.data_ptr(), dupv.stride(0), wd.data_ptr(), dxv.data_ptr(), dxv.stride(0),
         n, h, w, cin, cout, G.DT[dtype], G.stream())
    assert rel(G.from_nhwc(dxv, n, h, w), gx_ref) < TOL[dtype]
    nbytes = _lib.load().unetdc_convT2x2_wgrad_workspace(n, h, w, cin, cout, G.DT[dtype])
    ws = G.workspace(nbytes)
    dw = torch.full((cin, cout, 2, 2), float("nan"), device="cuda")
    call("unetdc_convT2x2_wgrad", xv.data_ptr(), xv.stride(0), dupv.data_ptr(), dupv.stride(0), dw.data_ptr(),
         ws.data_ptr(), nbytes, n, h, w, cin, cout, G.DT[dtype], G.stream())
    assert rel(dw.cpu(), gw_ref) < TOL_W[dtype]
    nb2 = _lib.load().unetdc_channel_sum_workspace(n * 4 * h * w, cout)
    ws2 = G.workspace(nb2)
    db = torch.full((cout,), float("nan"), device="cuda")
    call("unetdc_channel_sum", dupv.data_ptr(), dupv.stride(0), db.data_ptr(), ws2.data_ptr(), nb2, n * 4 * h * w,
         cout, G.DT[dtype], G.stream())
    assert rel(db.cpu(), gb_ref) < 1e-5


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("case", [(2, 16, 24, 64), (1, 8, 8, 1024), (3, 4, 4, 256)])
def test_bn_relu_fwd_bwd(dtype, pool, case):
    """conv-output y -> BatchNorm(train) -> ReLU -> {skip, max_pool2d}: forward and backward."""
    n, h, w, c = case
    g = gen(11)
    y = G.quant(torch.randn(n, c, h, w, generator=g) * 2 + 0.5, dtype)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    rm0, rv0 = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    dskip = G.quant(torch.randn(n, c, h, w, generator=g), dtype)
    dpool = G.quant(torch.randn(n, c, h // 2, w // 2, generator=g), dtype)
    # ---- reference (fp32 ATen); for bf16 the activation is rounded before pooling like the kernel
    yr, gr, br = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    a_ref = torch.relu(F.batch_norm(yr, rm, rv, gr, br, training=True, momentum=0.1, eps=1e-5))
    out = (a_ref * dskip).sum()
    if pool:
        # the pooling sees the activation as stored (rounded through the compute type); straight-through
        a_q = a_ref + (G.quant(a_ref.detach(), dtype) - a_ref.detach())
        out = out + (F.max_pool2d(a_q, 2) * dpool).sum()
    gy_ref, gg_ref, gb_ref = torch.autograd.grad(out, (yr, gr, br))
    # ---- HIP: statistics partials come from the conv epilogue; emulate one partial row here
    cnt = n * h * w
    part = torch.zeros((1 + 64) * 2 * c, device="cuda")
    yd = y.double()
    part[:c] = yd.sum(dim=(0, 2, 3)).float().cuda()
    part[c:2 * c] = (yd * yd).sum(dim=(0, 2, 3)).float().cuda()
    f32 = dict(device="cuda", dtype=torch.float32)
    scale, shift, mean, rstd = (torch.empty(c, **f32) for _ in range(4))
    rmd, rvd = rm0.cuda(), rv0.cuda()
    gd, bd = gamma.cuda(), beta.cuda()
    call("unetdc_bn_finalize", part.data_ptr(), 1, cnt, gd.data_ptr(), bd.data_ptr(), 1e-5, 0.1, rmd.data_ptr(),
         rvd.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), c, G.stream())
    np.testing.assert_allclose(rmd.cpu().numpy(), rm.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rvd.cpu().numpy(), rv.numpy(), rtol=1e-5, atol=1e-6)
    yv = G.to_nhwc(y, dtype)
    av = G.empty_nhwc(cnt, c, dtype, ld=2 * c, off=c)
    pv = G.empty_nhwc(cnt // 4, c, dtype) if pool else None
    call("unetdc_bn_relu_apply", yv.data_ptr(), yv.stride(0), scale.data_ptr(), shift.data_ptr(), av.data_ptr(),
         av.stride(0), None if pv is None else pv.data_ptr(), 0 if pv is None else pv.stride(0), n, h, w, c,
         G.DT[dtype], G.stream())
    a = G.from_nhwc(av, n, h, w)
    assert rel(a, a_ref.detach()) < (1e-5 if dtype == "f32" else 4e-3)
    if pool:
        np.testing.assert_array_equal(G.from_nhwc(pv, n, h // 2, w // 2).numpy(), F.max_pool2d(a, 2).numpy())
    # ---- backward
    nbytes = _lib.load().unetdc_bn_relu_bwd_workspace(n, h, w, c, int(pool), G.DT[dtype])
    ws = G.workspace(nbytes)
    dsv = G.to_nhwc(dskip, dtype, ld=2 * c, off=c)
    dpv = G.to_nhwc(dpool, dtype) if pool else None
    dyv = G.empty_nhwc(cnt, c, dtype)
    dgam, dbet, dbias = (torch.full((c,), float("nan"), **f32) for _ in range(3))
    call("unetdc_bn_relu_bwd", dsv.data_ptr(), dsv.stride(0), None if dpv is None else dpv.data_ptr(),
         0 if dpv is None else dpv.stride(0), yv.data_ptr(), yv.stride(0), scale.data_ptr(), shift.data_ptr(),
         mean.data_ptr(), rstd.data_ptr(), gd.data_ptr(), dyv.data_ptr(), dyv.stride(0), dgam.data_ptr(),
         dbet.data_ptr(), dbias.data_ptr(), ws.data_ptr(), nbytes, None, 0, n, h, w, c, G.DT[dtype], G.stream())
    tol = 2e-5 if dtype == "f32" else 2e-2      # bf16: relu/argmax decided on rounded activations
    assert rel(dgam.cpu(), gg_ref) < tol, ("dgamma", rel(dgam.cpu(), gg_ref))
    assert rel(dbet.cpu(), gb_ref) < tol, ("dbeta", rel(dbet.cpu(), gb_ref))
    assert rel(G.from_nhwc(dyv, n, h, w), gy_ref) < tol, ("dy", rel(G.from_nhwc(dyv, n, h, w), gy_ref))
    assert float(dbias.abs().max()) < 1e-2 * float(gb_ref.abs().max() + 1)     # ~0 by construction


@pytest.mark.parametrize("rows,c", [(1, 64), (37, 6), (512, 64), (700, 10), (300, 1024)])
def test_bn_finalize_many_partial_rows(rows, c):
    """unetdc_bn_finalize over `rows` partial rows of (sum, sum of squares): one workgroup per four channels, rows strided
    over its 256 threads, fp64 from the partial sums on -- also channel counts that are not a multiple of four and row counts
    beyond the 512 that go through the pre-reduction stage (nn.BatchNorm2d training statistics, models/model_2.py:45,52)."""
    g = gen(23)
    cnt = 4096 * rows
    part = torch.zeros((rows + 64) * 2 * c, dtype=torch.float32)
    pv = part[: rows * 2 * c].view(rows, 2, c)
    pv[:, 0] = torch.randn(rows, c, generator=g) * 30 + 100        # partial sums of ~4096 values each
    pv[:, 1] = torch.rand(rows, c, generator=g) * 4000 + 9000
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm0, rv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    s, q = pv[:, 0].double().sum(0), pv[:, 1].double().sum(0)
    mean = s / cnt
    var = (q / cnt - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    f32 = dict(device="cuda", dtype=torch.float32)
    pd = part.cuda()
    scale, shift, mean_d, rstd_d = (torch.full((c,), float("nan"), **f32) for _ in range(4))
    rmd, rvd, gd, bd = rm0.cuda(), rv0.cuda(), gamma.cuda(), beta.cuda()
    call("unetdc_bn_finalize", pd.data_ptr(), rows, cnt, gd.data_ptr(), bd.data_ptr(), 1e-5, 0.1, rmd.data_ptr(),
         rvd.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean_d.data_ptr(), rstd_d.data_ptr(), c, G.stream())
    rt = 1e-6 if rows <= 512 else 3e-6                      # > 512 rows: one fp32 pre-reduction stage in front
    np.testing.assert_allclose(mean_d.cpu().numpy(), mean.float().numpy(), rtol=rt, atol=1e-7)
    np.testing.assert_allclose(rstd_d.cpu().numpy(), rstd.float().numpy(), rtol=rt)
    np.testing.assert_allclose(scale.cpu().numpy(), (gamma.double() * rstd).float().numpy(), rtol=4e-6)
    np.testing.assert_allclose(shift.cpu().numpy(), (beta.double() - mean * gamma.double() * rstd).float().numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(rmd.cpu().numpy(), (0.9 * rm0.double() + 0.1 * mean).float().numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(rvd.cpu().numpy(), (0.9 * rv0.double() + 0.1 * var * cnt / (cnt - 1)).float().numpy(), rtol=2e-6)
    # bitwise reproducible: the summation order is fixed
    scale2 = torch.full((c,), float("nan"), **f32)
    call("unetdc_bn_finalize", pd.data_ptr(), rows, cnt, gd.data_ptr(), bd.data_ptr(), 1e-5, 0.1, None, None,
         scale2.data_ptr(), shift.data_ptr(), mean_d.data_ptr(), rstd_d.data_ptr(), c, G.stream())
    assert torch.equal(scale2, scale)


@pytest.mark.parametrize("case", [(2, 256, 256, 64, 64, 1), (3, 512, 256, 64, 64, 1), (2, 64, 256, 64, 64, 2), (2, 96, 192, 64, 64, 1),
                                  (2, 128, 128, 128, 64, 1),
                                  # 128-channel n-blocks (round 5: the wide lattice kernel normalises on load too, constants through SGPRs)
                                  (2, 128, 128, 128, 128, 1), (1, 128, 256, 256, 256, 1), (2, 64, 256, 128, 128, 2), (8, 64, 64, 512, 512, 1),
                                  (3, 64, 192, 128, 256, 1)])
def test_conv_and_wgrad_fed_from_raw_output_normalise_on_load(case):
    """unetdc_conv3x3_fwd_bnin / unetdc_conv3x3_wgrad_bnin (bf16): fed from the RAW output of the stage in front, they apply its
    BatchNorm + ReLU per staged tile in LDS.  Bit-identical to the two-pass form (unetdc_bn_relu_apply, then the plain
    kernels) -- output, statistics rows and weight gradient -- incl. image borders (zero padding of the ACTIVATION, not of
    the raw tensor), several items per workgroup, d = 2, two K chunks, strided views."""
    n, h, w, cin, cout, d = case
    dtype = "bf16"
    lib = _lib.load()
    mode = lib.unetdc_conv3x3_bnin_supported(n, h, w, cin, cout, d, G.DT[dtype])
    assert mode == (2 if cout % 128 == 0 else 1)        # 128-channel n-blocks: the forward can store the normalised activation
    g = gen(41)
    yraw = G.quant(torch.randn(n, cin, h, w, generator=g) * 1.5, dtype)
    sc, sh = (torch.rand(cin, generator=g) + 0.5).cuda(), (torch.randn(cin, generator=g) * 0.4 + 0.3).cuda()   # relu(shift) != 0
    wt = G.quant(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5), dtype)
    b = torch.randn(cout, generator=g).cuda()
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    wf, _ = G.pack_conv(wt, dtype)
    yv = G.to_nhwc(yraw, dtype, ld=cin + 64, off=64)
    av = G.empty_nhwc(n * h * w, cin, dtype)
    call("unetdc_bn_relu_apply", yv.data_ptr(), yv.stride(0), sc.data_ptr(), sh.data_ptr(), av.data_ptr(), av.stride(0), None, 0,
         n, h, w, cin, G.DT[dtype], G.stream())
    # forward: two passes vs normalise-on-load
    o_ref = G.empty_nhwc(n * h * w, cout, dtype)
    st_ref, rows = G.conv3x3_fwd(av, wf, b, n, h, w, cin, cout, d, dtype, o_ref, stats=True)
    live_ref = G.LIVE_ROWS.value
    o = G.empty_nhwc(n * h * w, cout, dtype)
    st = torch.full_like(st_ref, float("nan"))
    live = ctypes.c_int(-1)
    act = G.empty_nhwc(n * h * w, cin, dtype, ld=cin + 64, off=32) if mode == 2 else None      # (strided view, NaN-filled)
    call("unetdc_conv3x3_fwd_bnin", yv.data_ptr(), yv.stride(0), sc.data_ptr(), sh.data_ptr(), wf.data_ptr(), b.data_ptr(),
         o.data_ptr(), o.stride(0), st.data_ptr(), ctypes.byref(live), None if act is None else act.data_ptr(),
         0 if act is None else act.stride(0), n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    assert lib.unetdc_last_kernel().decode().endswith("bnin")
    assert live.value == live_ref >= 1
    assert torch.equal(o, o_ref)
    assert torch.equal(st[: rows * 2 * cout], st_ref[: rows * 2 * cout])
    if act is not None:
        assert torch.equal(act, av)                     # the stored activation == what the stand-alone pass writes, bit for bit
    else:                                               # the 64-channel form has no write-back: asking for one is refused
        with pytest.raises(_lib.UnetdcError, match="stores the activation"):
            call("unetdc_conv3x3_fwd_bnin", yv.data_ptr(), yv.stride(0), sc.data_ptr(), sh.data_ptr(), wf.data_ptr(), b.data_ptr(),
                 o.data_ptr(), o.stride(0), st.data_ptr(), ctypes.byref(live), av.data_ptr(), av.stride(0), n, h, w, cin, cout, d,
                 G.DT[dtype], G.stream())
    # weight gradient
    dyv = G.to_nhwc(dy, dtype)
    dw_ref = G.conv3x3_wgrad(av, dyv, n, h, w, cin, cout, d, dtype)
    nbytes = lib.unetdc_conv3x3_wgrad_workspace(n, h, w, cin, cout, G.DT[dtype])
    ws = G.workspace(nbytes)
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    call("unetdc_conv3x3_wgrad_bnin", yv.data_ptr(), yv.stride(0), sc.data_ptr(), sh.data_ptr(), dyv.data_ptr(), dyv.stride(0),
         dw.data_ptr(), ws.data_ptr(), nbytes, n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    assert lib.unetdc_last_kernel().decode().endswith("bnin")
    assert torch.equal(dw, dw_ref)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("shape", [(2, 24, 40, 1), (1, 64, 64, 2), (3, 10, 10, 1), (1, 8, 8, 16)])
def test_first_conv_input_gradient(dtype, cin, shape):
    """unetdc_conv3x3_first_dgrad: dL/dx of the first convolution vs torch autograd (ragged maps, dilation, a dilation
    larger than the map: only the centre tap is in bounds)."""
    n, h, w, d = shape
    cout = 64
    g = gen(31)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / 3
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    xr = torch.zeros(n, cin, h, w, requires_grad=True)
    dx_ref, = torch.autograd.grad(F.conv2d(xr, wt, None, padding=d, dilation=d), xr, dy)
    dyv = G.to_nhwc(dy, dtype, ld=cout + 64, off=64)         # strided view
    wd_, dx = wt.cuda().contiguous(), torch.full((n, cin, h, w), float("nan"), device="cuda")
    call("unetdc_conv3x3_first_dgrad", dyv.data_ptr(), dyv.stride(0), wd_.data_ptr(), dx.data_ptr(), n, h, w, cin, cout, d,
         G.DT[dtype], G.stream())
    assert rel(dx.cpu(), dx_ref) < 2e-5            # fp32 accumulate of exactly representable operands on both sides


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("oc", [1, 2])
def test_head_fwd_bwd(dtype, oc):
    n, h, w, c = 2, 16, 24, 64
    g = gen(13)
    a = G.quant(torch.rand(n, c, h, w, generator=g), dtype)
    wt = torch.randn(oc, c, 1, 1, generator=g) * 0.3
    b = torch.randn(oc, generator=g) * 0.1
    dp = torch.randn(n, oc, h, w, generator=g)
    ar, wr, br = a.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    p_ref = torch.sigmoid(F.conv2d(ar, wr, br))
    ga_ref, gw_ref, gb_ref = torch.autograd.grad(p_ref, (ar, wr, br), dp)
    av = G.to_nhwc(a, dtype)
    probs = torch.full((n, oc, h, w), float("nan"), device="cuda")
    wd2, bd2 = wt.reshape(oc, c).cuda().contiguous(), b.cuda()
    call("unetdc_head_fwd", av.data_ptr(), av.stride(0), wd2.data_ptr(), bd2.data_ptr(), probs.data_ptr(), n, h, w, c,
         oc, G.DT[dtype], G.stream())
    assert float((probs.cpu() - p_ref.detach()).abs().max()) < 2e-6
    nbytes = _lib.load().unetdc_head_bwd_workspace(n, h, w, c, oc, G.DT[dtype])
    ws = G.workspace(nbytes)
    dav = G.empty_nhwc(n * h * w, c, dtype)
    dw, db = torch.full((oc, c), float("nan"), device="cuda"), torch.full((oc,), float("nan"), device="cuda")
    dpd = dp.cuda()
    call("unetdc_head_bwd", dpd.data_ptr(), probs.data_ptr(), av.data_ptr(), av.stride(0), wd2.data_ptr(),
         dav.data_ptr(), dav.stride(0), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, n, h, w, c, oc,
         G.DT[dtype], G.stream())
    assert rel(dw.cpu().reshape(oc, c, 1, 1), gw_ref) < 2e-5
    assert rel(db.cpu(), gb_ref) < 2e-5
    assert rel(G.from_nhwc(dav, n, h, w), ga_ref) < (1e-5 if dtype == "f32" else (4e-3 if oc == 1 else 8e-3))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 24, 1), (1, 64, 64, 1), (3, 160, 96, 2)])
def test_head_bwd_fused_bn_backward_sums(dtype, shape):
    """unetdc_head_bwd_bnstats: same da (bitwise) / dw / db as unetdc_head_bwd, and partial rows whose column sums are the
    BatchNorm-backward sums S1 = sum dyhat, S2 = sum dyhat * xhat, S3 = sum xhat of the stored gradient (fp64 restatement
    of csrc/batchnorm.hip bn_bwd_kernel on the device's own da and y)."""
    import ctypes
    n, h, w, oc = shape
    c = 64
    g = gen(29)
    y = G.quant(torch.randn(n, c, h, w, generator=g), dtype)
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    mean, rstd = torch.randn(c, generator=g) * 0.2, torch.rand(c, generator=g) + 0.5
    a = G.quant(torch.relu(y * scale.view(1, c, 1, 1) + shift.view(1, c, 1, 1)), dtype)
    wt = torch.randn(oc, c, generator=g) * 0.3
    probs = torch.rand(n, oc, h, w, generator=g).cuda()
    dp = torch.randn(n, oc, h, w, generator=g).cuda()
    av, yv = G.to_nhwc(a, dtype), G.to_nhwc(y, dtype)
    wd2 = wt.cuda().contiguous()
    nbytes = _lib.load().unetdc_head_bwd_workspace(n, h, w, c, oc, G.DT[dtype])
    ws = G.workspace(nbytes)
    outs = []
    rows = _lib.load().unetdc_conv3x3_stats_rows(n * h * w, c)
    parts = torch.full(((rows + 64) * 3 * c,), float("nan"), device="cuda")
    dv = [t.cuda() for t in (scale, shift, mean, rstd)]
    npar = ctypes.c_int(0)
    # normalise-on-load forward: the head fed from the raw conv output == the head fed from the activation the stand-alone
    # pass stores (unetdc_bn_relu_apply: the same fused multiply-add and rounding), bit for bit
    av = G.empty_nhwc(n * h * w, c, dtype)
    call("unetdc_bn_relu_apply", yv.data_ptr(), yv.stride(0), dv[0].data_ptr(), dv[1].data_ptr(), av.data_ptr(), av.stride(0),
         None, 0, n, h, w, c, G.DT[dtype], G.stream())
    bd2 = (torch.randn(oc, generator=g) * 0.1).cuda()
    p_a, p_y = (torch.full((n, oc, h, w), float("nan"), device="cuda") for _ in range(2))
    call("unetdc_head_fwd", av.data_ptr(), av.stride(0), wd2.data_ptr(), bd2.data_ptr(), p_a.data_ptr(), n, h, w, c, oc,
         G.DT[dtype], G.stream())
    call("unetdc_head_fwd_bn", yv.data_ptr(), yv.stride(0), dv[0].data_ptr(), dv[1].data_ptr(), wd2.data_ptr(), bd2.data_ptr(),
         p_y.data_ptr(), n, h, w, c, oc, G.DT[dtype], G.stream())
    assert torch.equal(p_a, p_y)
    for fused in (False, True, "from_y"):
        dav = G.empty_nhwc(n * h * w, c, dtype)
        dw, db = torch.full((oc, c), float("nan"), device="cuda"), torch.full((oc,), float("nan"), device="cuda")
        if fused == "from_y":                            # a == NULL: the activation is recomputed from y / scale / shift
            call("unetdc_head_bwd_bnstats", dp.data_ptr(), probs.data_ptr(), None, c, wd2.data_ptr(),
                 dav.data_ptr(), dav.stride(0), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, yv.data_ptr(),
                 yv.stride(0), dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), parts.data_ptr(),
                 parts.numel(), ctypes.byref(npar), n, h, w, c, oc, G.DT[dtype], G.stream())
        elif fused:
            call("unetdc_head_bwd_bnstats", dp.data_ptr(), probs.data_ptr(), av.data_ptr(), av.stride(0), wd2.data_ptr(),
                 dav.data_ptr(), dav.stride(0), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, yv.data_ptr(),
                 yv.stride(0), dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), parts.data_ptr(),
                 parts.numel(), ctypes.byref(npar), n, h, w, c, oc, G.DT[dtype], G.stream())
        else:
            call("unetdc_head_bwd", dp.data_ptr(), probs.data_ptr(), av.data_ptr(), av.stride(0), wd2.data_ptr(),
                 dav.data_ptr(), dav.stride(0), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, n, h, w, c, oc,
                 G.DT[dtype], G.stream())
        torch.cuda.synchronize()
        outs.append((dav.clone(), dw.clone(), db.clone()))
    assert torch.equal(outs[0][0], outs[1][0])               # da: bitwise
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1]) and torch.equal(outs[1][2], outs[2][2])
    for u, v in zip(outs[0][1:], outs[1][1:]):               # dw, db: the fused launch may take fewer workgroups (rows of `parts`)
        assert rel(u.cpu(), v.cpu()) < 1e-5
    assert 1 <= npar.value <= rows + 64
    got = parts[: npar.value * 3 * c].view(npar.value, 3, c).double().sum(0).cpu()
    da = outs[1][0].double().cpu()[:, :c]                      # [pixels][c], as stored
    yy = yv.double().cpu()[:, :c]
    gate = (yy * scale.double() + shift.double()) > 0           # sign of the exact value = sign of the kernel's fp32 fma
    gh = torch.where(gate, da, torch.zeros_like(da))
    xh = (yy - mean.double()) * rstd.double()
    ref = torch.stack([gh.sum(0), (gh * xh).sum(0), xh.sum(0)])
    tol = 2e-5 * (ref.abs().max() + (gh.abs().sum(0).max()))
    assert float((got - ref).abs().max()) < float(tol), float((got - ref).abs().max())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 24), (1, 64, 64), (3, 160, 96)])
def test_bn_backward_recomputes_the_head_gradient(dtype, shape):
    """unetdc_head_bwd_bnstats with da = NULL + unetdc_bn_relu_bwd_head (one-channel head, models/model_2.py:76-80): the
    gradient of the head's input is recomputed per pixel instead of stored -- dy, dgamma, dbeta, dbias and the head's own
    dw / db are BIT-identical to the stored form (unetdc_head_bwd_bnstats with da + unetdc_bn_relu_bwd)."""
    import ctypes
    n, h, w = shape
    c, oc = 64, 1
    g = gen(31)
    y = G.quant(torch.randn(n, c, h, w, generator=g), dtype)
    gamma = torch.rand(c, generator=g) + 0.5
    mean, rstd = torch.randn(c, generator=g) * 0.2, torch.rand(c, generator=g) + 0.5
    scale = gamma * rstd
    shift = torch.randn(c, generator=g) * 0.3 - mean * scale
    wt = (torch.randn(oc, c, generator=g) * 0.3).cuda().contiguous()
    probs = torch.rand(n, oc, h, w, generator=g).cuda()
    dp = torch.randn(n, oc, h, w, generator=g).cuda()
    yv = G.to_nhwc(y, dtype)
    dv = [t.cuda() for t in (scale, shift, mean, rstd, gamma)]
    nbytes = _lib.load().unetdc_head_bwd_workspace(n, h, w, c, oc, G.DT[dtype])
    ws = G.workspace(nbytes)
    nb2 = _lib.load().unetdc_bn_relu_bwd_workspace(n, h, w, c, 0, G.DT[dtype])
    ws2 = G.workspace(nb2)
    rows = _lib.load().unetdc_conv3x3_stats_rows(n * h * w, c)
    f32 = dict(device="cuda", dtype=torch.float32)
    res = []
    for stored in (True, False):
        parts = torch.full(((rows + 64) * 3 * c,), float("nan"), device="cuda")
        npar = ctypes.c_int(0)
        dav = G.empty_nhwc(n * h * w, c, dtype)
        dw, db = torch.full((oc, c), float("nan"), **f32), torch.full((oc,), float("nan"), **f32)
        call("unetdc_head_bwd_bnstats", dp.data_ptr(), probs.data_ptr(), None, c, wt.data_ptr(),
             dav.data_ptr() if stored else None, dav.stride(0), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes,
             yv.data_ptr(), yv.stride(0), dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(),
             parts.data_ptr(), parts.numel(), ctypes.byref(npar), n, h, w, c, oc, G.DT[dtype], G.stream())
        dyv = G.empty_nhwc(n * h * w, c, dtype)
        dgam, dbet, dbias = (torch.full((c,), float("nan"), **f32) for _ in range(3))
        if stored:
            call("unetdc_bn_relu_bwd", dav.data_ptr(), dav.stride(0), None, 0, yv.data_ptr(), yv.stride(0), dv[0].data_ptr(),
                 dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), dyv.data_ptr(), dyv.stride(0),
                 dgam.data_ptr(), dbet.data_ptr(), dbias.data_ptr(), ws2.data_ptr(), nb2, parts.data_ptr(), npar.value,
                 n, h, w, c, G.DT[dtype], G.stream())
        else:
            call("unetdc_bn_relu_bwd_head", dp.data_ptr(), probs.data_ptr(), wt.data_ptr(), yv.data_ptr(), yv.stride(0),
                 dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), dyv.data_ptr(),
                 dyv.stride(0), dgam.data_ptr(), dbet.data_ptr(), dbias.data_ptr(), ws2.data_ptr(), nb2, parts.data_ptr(),
                 npar.value, n, h, w, c, G.DT[dtype], G.stream())
        torch.cuda.synchronize()
        res.append([t.clone() for t in (dyv, dgam, dbet, dbias, dw, db)])
    for a, b in zip(*res):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    # and it is the right gradient: dy against autograd of relu(batch_norm) on the CPU for the incoming gradient dz * w
    dz = (dp * probs * (1 - probs)).cpu()
    da_ref = G.quant(dz * wt.cpu().view(1, c, 1, 1), dtype)
    yr = y.clone().requires_grad_(True)
    a_ref = torch.relu((yr - mean.view(1, c, 1, 1)) * rstd.view(1, c, 1, 1) * gamma.view(1, c, 1, 1)
                       + (shift + mean * scale).view(1, c, 1, 1))
    gate = (a_ref > 0).float()
    gh = da_ref * gate
    xh = ((y - mean.view(1, c, 1, 1)) * rstd.view(1, c, 1, 1)).double()
    m = n * h * w
    k1 = (gamma * rstd).double().view(1, c, 1, 1)
    dy_ref = k1 * (gh.double() - gh.double().sum((0, 2, 3), keepdim=True) / m
                   - xh * (gh.double() * xh).sum((0, 2, 3), keepdim=True) / m)
    assert rel(G.from_nhwc(res[1][0], n, h, w), dy_ref.float()) < (2e-5 if dtype == "f32" else 8e-3)
    with pytest.raises(_lib.UnetdcError, match="da may be NULL only"):
        call("unetdc_head_bwd_bnstats", dp.data_ptr(), probs.data_ptr(), None, c, wt.data_ptr(), None, c, dw.data_ptr(),
             db.data_ptr(), ws.data_ptr(), nbytes, yv.data_ptr(), yv.stride(0), dv[0].data_ptr(), dv[1].data_ptr(),
             dv[2].data_ptr(), dv[3].data_ptr(), parts.data_ptr(), parts.numel(), ctypes.byref(npar), n, h, w, c, 2,
             G.DT[dtype], G.stream())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 24), (1, 64, 64), (3, 40, 96)])
def test_first_wgrad_applies_batchnorm_backward_on_load(dtype, shape):
    """unetdc_bn_relu_bwd_coeffs + unetdc_conv3x3_first_wgrad_bn (enc1.0 with one input channel, models/model_2.py:10,41-46
    under autograd) == unetdc_bn_relu_bwd + unetdc_conv3x3_first_wgrad, bit for bit: dw, dgamma, dbeta, dbias."""
    n, h, w = shape
    cin, c = 1, 64
    assert _lib.load().unetdc_conv3x3_first_wgrad_bn_supported(n, h, w, cin, c, 1, G.DT[dtype]) == 1
    assert _lib.load().unetdc_conv3x3_first_wgrad_bn_supported(n, h, w, 3, c, 1, G.DT[dtype]) == 0
    g = gen(37)
    x = torch.randn(n, cin, h, w, generator=g).cuda().contiguous()
    y = G.quant(torch.randn(n, c, h, w, generator=g), dtype)
    dz = G.quant(torch.randn(n, c, h, w, generator=g), dtype)
    gamma = torch.rand(c, generator=g) + 0.5
    mean, rstd = torch.randn(c, generator=g) * 0.2, torch.rand(c, generator=g) + 0.5
    scale = gamma * rstd
    shift = torch.randn(c, generator=g) * 0.3 - mean * scale
    yv, dzv = G.to_nhwc(y, dtype), G.to_nhwc(dz, dtype)
    dv = [t.cuda() for t in (scale, shift, mean, rstd, gamma)]
    # the sums a fused dgrad epilogue would have left, as two partial rows
    yq, dq = yv.float().cpu()[:, :c].double(), dzv.float().cpu()[:, :c].double()
    gate = (yq * scale.double() + shift.double()) > 0
    xh = (yq - mean.double()) * rstd.double()
    gh = torch.where(gate, dq, torch.zeros_like(dq))
    rows = 2
    parts = torch.zeros((rows + 64) * 3 * c, device="cuda")
    pv = parts[: rows * 3 * c].view(rows, 3, c)
    for r in range(rows):
        sel = slice(r, None, rows)
        pv[r, 0], pv[r, 1], pv[r, 2] = gh[sel].sum(0).float().cuda(), (gh[sel] * xh[sel]).sum(0).float().cuda(), xh[sel].sum(0).float().cuda()
    f32 = dict(device="cuda", dtype=torch.float32)
    nb = _lib.load().unetdc_bn_relu_bwd_workspace(n, h, w, c, 0, G.DT[dtype])
    ws = G.workspace(nb)
    nbw = _lib.load().unetdc_conv3x3_first_wgrad_workspace(n, h, w, cin, c)
    wsw = G.workspace(nbw)
    # two-pass form
    dyv = G.empty_nhwc(n * h * w, c, dtype)
    a = [torch.full((c,), float("nan"), **f32) for _ in range(3)]
    call("unetdc_bn_relu_bwd", dzv.data_ptr(), dzv.stride(0), None, 0, yv.data_ptr(), yv.stride(0), dv[0].data_ptr(),
         dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), dv[4].data_ptr(), dyv.data_ptr(), dyv.stride(0), a[0].data_ptr(),
         a[1].data_ptr(), a[2].data_ptr(), ws.data_ptr(), nb, parts.data_ptr(), rows, n, h, w, c, G.DT[dtype], G.stream())
    dw_a = torch.full((c, cin, 3, 3), float("nan"), **f32)
    call("unetdc_conv3x3_first_wgrad", x.data_ptr(), dyv.data_ptr(), dyv.stride(0), dw_a.data_ptr(), wsw.data_ptr(), nbw,
         n, h, w, cin, c, 1, G.DT[dtype], G.stream())
    # on-load form
    b = [torch.full((c,), float("nan"), **f32) for _ in range(3)]
    coef = torch.full((3 * c,), float("nan"), **f32)
    call("unetdc_bn_relu_bwd_coeffs", parts.data_ptr(), rows, dv[4].data_ptr(), dv[3].data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
         b[2].data_ptr(), coef.data_ptr(), n, h, w, c, G.stream())
    dw_b = torch.full((c, cin, 3, 3), float("nan"), **f32)
    call("unetdc_conv3x3_first_wgrad_bn", x.data_ptr(), dzv.data_ptr(), dzv.stride(0), yv.data_ptr(), yv.stride(0),
         dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), coef.data_ptr(), dw_b.data_ptr(), wsw.data_ptr(),
         nbw, n, h, w, cin, c, 1, G.DT[dtype], G.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(dw_b).all() and torch.equal(dw_a, dw_b)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # and dw is the weight gradient of the convolution for that dy (CPU fp32 reference)
    dy_ref = G.from_nhwc(dyv, n, h, w)
    wref = torch.zeros(c, cin, 3, 3, requires_grad=True)
    F.conv2d(x.cpu(), wref, padding=1).backward(dy_ref)
    assert rel(dw_b.cpu(), wref.grad) < 1e-4


def test_argument_errors_are_reported():
    """Error behaviour of the boundary: bad shapes return a negative code + message, no crash."""
    x = torch.zeros(64, 48, device="cuda")
    with pytest.raises(_lib.UnetdcError, match="multiple of"):
        call("unetdc_conv3x3_fwd", x.data_ptr(), 48, x.data_ptr(), None, None, None, x.data_ptr(), 64, None, None,
             1, 8, 8, 48, 64, 1, _lib.F32, G.stream())
    with pytest.raises(_lib.UnetdcError, match="workspace too small"):
        call("unetdc_conv3x3_wgrad", x.data_ptr(), 64, x.data_ptr(), 64, x.data_ptr(), x.data_ptr(), 16,
             1, 8, 8, 64, 64, 1, _lib.F32, G.stream())


def _tight_case(name):
    """(query bytes, NaN-prefilled outputs, run(workspace pointer, bytes)) of one workspace-taking call at a tiny shape."""
    lib, g = _lib.load(), gen(41)
    f32 = dict(device="cuda", dtype=torch.float32)
    nan = lambda *shape: torch.full(shape, float("nan"), **f32)
    if name.startswith("bn_relu_bwd"):
        n, h, w, c, pool, dtype = (1, 4, 6, 16, True, "f32") if name.endswith("pooled") else (1, 4, 4, 8, False, "bf16")
        yv = G.to_nhwc(torch.randn(n, c, h, w, generator=g), dtype)
        dsv = G.to_nhwc(torch.randn(n, c, h, w, generator=g), dtype)
        dpv = G.to_nhwc(torch.randn(n, c, h // 2, w // 2, generator=g), dtype) if pool else None
        sc, sh, mu, rs, ga = ((torch.rand(c, generator=g) + 0.5).cuda() for _ in range(5))
        outs = [G.empty_nhwc(n * h * w, c, dtype), nan(c), nan(c), nan(c)]
        nbytes = lib.unetdc_bn_relu_bwd_workspace(n, h, w, c, int(pool), G.DT[dtype])
        run = lambda ws, nb: call("unetdc_bn_relu_bwd", dsv.data_ptr(), dsv.stride(0), dpv.data_ptr() if pool else None,
                                  dpv.stride(0) if pool else 0, yv.data_ptr(), yv.stride(0), sc.data_ptr(), sh.data_ptr(),
                                  mu.data_ptr(), rs.data_ptr(), ga.data_ptr(), outs[0].data_ptr(), outs[0].stride(0),
                                  outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), ws, nb, None, 0, n, h, w, c,
                                  G.DT[dtype], G.stream())
    elif name.startswith("head_bwd"):
        n, h, w, c, oc, dtype = (1, 4, 4, 8, 2, "f32") if name.endswith("oc2") else (1, 4, 4, 8, 1, "bf16")
        av = G.to_nhwc(torch.randn(n, c, h, w, generator=g), dtype)
        probs, dp = torch.rand(n, oc, h, w, generator=g).cuda(), torch.randn(n, oc, h, w, generator=g).cuda()
        wt = torch.randn(oc, c, generator=g).cuda()
        outs = [G.empty_nhwc(n * h * w, c, dtype), nan(oc, c), nan(oc)]
        nbytes = lib.unetdc_head_bwd_workspace(n, h, w, c, oc, G.DT[dtype])
        run = lambda ws, nb: call("unetdc_head_bwd", dp.data_ptr(), probs.data_ptr(), av.data_ptr(), av.stride(0), wt.data_ptr(),
                                  outs[0].data_ptr(), outs[0].stride(0), outs[1].data_ptr(), outs[2].data_ptr(), ws, nb, n, h, w,
                                  c, oc, G.DT[dtype], G.stream())
    elif name == "channel_sum":
        npix, c, dtype = 48, 8, "f32"
        xv = G.to_nhwc(torch.randn(1, c, 6, 8, generator=g), dtype)
        outs = [nan(c)]
        nbytes = lib.unetdc_channel_sum_workspace(npix, c)
        run = lambda ws, nb: call("unetdc_channel_sum", xv.data_ptr(), xv.stride(0), outs[0].data_ptr(), ws, nb, npix, c,
                                  G.DT[dtype], G.stream())
    else:
        n, h, w, cin, cout, dtype = 1, 8, 8, 64, 64, "bf16"
        dyv = G.to_nhwc(torch.randn(n, cout, h, w, generator=g), dtype)
        _, wd = G.pack_conv(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5), dtype)
        outs = [G.empty_nhwc(n * h * w, cin, dtype), nan(cin // 2)]
        nbytes = lib.unetdc_conv3x3_dgrad_colsum_workspace(n, h, w, cin)
        run = lambda ws, nb: call("unetdc_conv3x3_dgrad_colsum", dyv.data_ptr(), dyv.stride(0), wd.data_ptr(), outs[0].data_ptr(),
                                  outs[0].stride(0), outs[1].data_ptr(), 0, cin // 2, ws, nb, n, h, w, cin, cout, 1, G.DT[dtype],
                                  G.stream())
    return nbytes, outs, run


@pytest.mark.parametrize("name", ["bn_relu_bwd", "bn_relu_bwd_pooled", "head_bwd", "head_bwd_oc2", "channel_sum", "dgrad_colsum"])
def test_workspace_query_is_tight_and_a_short_workspace_is_refused(name):
    """What a *_workspace query answers is enough and is enforced.  With exactly the queried bytes (a stale, NaN-filled workspace
    with a guard band behind it) the outputs are bit-equal to the same call with 1 MiB, and the guard band is untouched; with one
    byte less the call raises "workspace too small" before any launch: the NaN-prefilled outputs stay as they were."""
    bits = lambda t: t.contiguous().view(torch.uint8).cpu()
    nbytes, outs, run = _tight_case(name)
    assert 0 < nbytes < (1 << 20)
    big = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device="cuda")
    run(big.data_ptr(), big.numel())
    ref = [bits(o) for o in outs]
    assert not any(bool(torch.isnan(o.float()).any()) for o in outs)
    nbytes2, outs, run = _tight_case(name)                                  # the same seeded inputs, fresh NaN outputs
    assert nbytes2 == nbytes
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0xA5
    run(ws.data_ptr(), nbytes)
    assert all(torch.equal(bits(o), r) for o, r in zip(outs, ref))
    assert bool((ws[nbytes:] == 0xA5).all()), "wrote past the queried bytes"
    _, outs, run = _tight_case(name)
    with pytest.raises(_lib.UnetdcError, match="workspace too small"):
        run(ws.data_ptr(), nbytes - 1)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o.float()).all()) for o in outs)


def test_pack_many_matches_per_layer_packers():
    """The single-launch tiled packer writes the same images as the per-layer packers."""
    import numpy as np
    g = gen(17)
    convs = [torch.randn(64, 64, 3, 3, generator=g), torch.randn(128, 64, 3, 3, generator=g), torch.randn(64, 256, 3, 3, generator=g)]
    cts = [torch.randn(128, 64, 2, 2, generator=g), torch.randn(256, 128, 2, 2, generator=g)]
    for dtype in ("f32", "bf16"):
        ent = []
        for wt in convs:
            wf, wd = G.pack_conv(wt, dtype)
            ent.append((wt.cuda().contiguous(), wf, wd, wt.shape[0], wt.shape[1], 0))
        for wt in cts:
            wf, wd = G.pack_convT(wt, dtype)
            ent.append((wt.cuda().contiguous(), wf, wd, wt.shape[0], wt.shape[1], 1))
        dt = np.dtype([("w", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("begin", "<i8"), ("a", "<i4"), ("b", "<i4"),
                       ("kind", "<i4"), ("pad", "<i4")])
        tab = np.zeros(len(ent), dtype=dt)
        outs, off = [], 0
        for i, (w, wf, wd, a, b, kind) in enumerate(ent):
            of, od = torch.zeros_like(wf), torch.zeros_like(wd)
            outs.append((of, od))
            tab[i] = (w.data_ptr(), of.data_ptr(), od.data_ptr(), off, a, b, kind, 0)
            off += (a // 32) * (b // 32)
        tdev = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        call("unetdc_pack_many", tdev.data_ptr(), len(ent), off, G.DT[dtype], G.stream())
        torch.cuda.synchronize()
        for (w, wf, wd, *_), (of, od) in zip(ent, outs):
            assert torch.equal(of, wf) and torch.equal(od, wd)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 16, 24, 64, 64, 1), (1, 32, 32, 128, 256, 4), (2, 256, 256, 64, 64, 1),
                                  (1, 512, 256, 128, 64, 2), (2, 96, 160, 64, 64, 1), (2, 48, 80, 128, 128, 1),
                                  (2, 128, 128, 256, 128, 1), (3, 512, 256, 64, 64, 1), (1, 128, 128, 128, 128, 4),
                                  (4, 32, 32, 256, 256, 16), (2, 48, 64, 128, 64, 16)])   # d = 16: 16 x 16 block order (bf16)
def test_dgrad_with_fused_bn_backward_statistics(dtype, case):
    """conv dgrad whose epilogue also emits the BatchNorm-backward partial sums of the consuming stage
    (S1 = sum dx*[n>0], S2 = sum dx*[n>0]*xhat), and bn_relu_bwd consuming them instead of its own pass."""
    import ctypes
    n, h, w, cin, cout, d = case
    g = gen(19)
    wt = G.quant(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5), dtype)
    dy = G.quant(torch.randn(n, cout, h, w, generator=g), dtype)
    yprev = G.quant(torch.randn(n, cin, h, w, generator=g) * 1.5 + 0.3, dtype)      # saved conv output of the consumer
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.2
    xr = torch.zeros(n, cin, h, w, requires_grad=True)
    dx_ref, = torch.autograd.grad(F.conv2d(xr, wt, None, padding=d, dilation=d), xr, dy)
    yd = yprev.double()
    mean, var = yd.mean(dim=(0, 2, 3)), yd.var(dim=(0, 2, 3), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    scale, shift = gamma.double() * rstd, beta.double() - mean * gamma.double() * rstd
    _, wd = G.pack_conv(wt, dtype)
    dyv, dxv, ypv = G.to_nhwc(dy, dtype), G.empty_nhwc(n * h * w, cin, dtype), G.to_nhwc(yprev, dtype)
    dev = lambda t_: t_.float().cuda()      # noqa: E731
    sc, sh, mu, rs = dev(scale), dev(shift), dev(mean), dev(rstd)
    rows = _lib.load().unetdc_conv3x3_stats_rows(n * h * w, cin)
    parts = torch.full(((rows + 64) * 3 * cin,), float("nan"), device="cuda")
    npart = ctypes.c_int(0)
    call("unetdc_conv3x3_dgrad_bnstats", dyv.data_ptr(), dyv.stride(0), wd.data_ptr(), dxv.data_ptr(), dxv.stride(0),
         ypv.data_ptr(), ypv.stride(0), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr(), parts.data_ptr(),
         parts.numel(), ctypes.byref(npart), n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    dx = G.from_nhwc(dxv, n, h, w)
    assert rel(dx, dx_ref) < TOL[dtype]
    # expected sums from the STORED dx (what bn_relu_bwd would read) -- fp64
    nrm = yd * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    gh = torch.where(nrm > 0, dx.double(), torch.zeros_like(nrm))
    xh = (yd - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
    pc = parts.cpu()[: npart.value * 3 * cin].reshape(npart.value, 3, cin).double().sum(0)
    tol = 2e-4 if dtype == "f32" else 2e-2
    s1, s2 = gh.sum(dim=(0, 2, 3)), (gh * xh).sum(dim=(0, 2, 3))
    assert float((pc[0] - s1).abs().max()) <= tol * float(gh.abs().sum(dim=(0, 2, 3)).max())
    assert float((pc[1] - s2).abs().max()) <= tol * float((gh * xh).abs().sum(dim=(0, 2, 3)).max())
    # third row: the fused epilogue writes exact zeros (sum of xhat vanishes for batch statistics); the stand-alone
    # reduction behind the first-generation kernels accumulates sum(xhat) itself
    if float(pc[2].abs().max()) != 0.0:
        s3 = xh.sum(dim=(0, 2, 3))
        assert float((pc[2] - s3).abs().max()) <= tol * float(xh.abs().sum(dim=(0, 2, 3)).max())
    # bn_relu_bwd with the precomputed partial sums == bn_relu_bwd doing its own reduction
    f32 = dict(device="cuda", dtype=torch.float32)
    gd = gamma.cuda()
    outs = []
    for pre in (None, parts):
        nbytes = _lib.load().unetdc_bn_relu_bwd_workspace(n, h, w, cin, 0, G.DT[dtype])
        ws = G.workspace(nbytes)
        o = G.empty_nhwc(n * h * w, cin, dtype)
        dgam, dbet, dbias = (torch.full((cin,), float("nan"), **f32) for _ in range(3))
        call("unetdc_bn_relu_bwd", dxv.data_ptr(), dxv.stride(0), None, 0, ypv.data_ptr(), ypv.stride(0), sc.data_ptr(),
             sh.data_ptr(), mu.data_ptr(), rs.data_ptr(), gd.data_ptr(), o.data_ptr(), o.stride(0), dgam.data_ptr(),
             dbet.data_ptr(), dbias.data_ptr(), ws.data_ptr(), nbytes, None if pre is None else pre.data_ptr(),
             0 if pre is None else npart.value, n, h, w, cin, G.DT[dtype], G.stream())
        outs.append((o.float().cpu(), dgam.cpu(), dbet.cpu()))
    assert rel(outs[1][0], outs[0][0]) < (1e-5 if dtype == "f32" else 4e-3)
    assert rel(outs[1][1], outs[0][1]) < 1e-4 and rel(outs[1][2], outs[0][2]) < 1e-4


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 16, 24, 128, 64, 1), (1, 64, 64, 256, 128, 1), (2, 256, 256, 128, 64, 1)])
def test_dgrad_with_fused_column_sums(dtype, case):
    """conv3x3_dgrad_colsum == conv3x3_dgrad (bitwise) + per-channel sums of the first half of the STORED result
    (the ConvTranspose2d bias gradient, torch: dcat[:, :C].sum over pixels), fp64 check of the sums."""
    n, h, w, cin, cout, d = case
    g = gen(17)
    P = n * h * w
    dyv = G.to_nhwc(torch.randn(n, cout, h, w, generator=g), dtype)
    _, wd = G.pack_conv(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5), dtype)
    dx0 = G.empty_nhwc(P, cin, dtype)
    G.conv3x3_dgrad(dyv, wd, dx0, n, h, w, cin, cout, d, dtype)
    dx1 = G.empty_nhwc(P, cin, dtype)
    c = cin // 2
    out = torch.full((c,), float("nan"), device="cuda")
    nbytes = _lib.load().unetdc_conv3x3_dgrad_colsum_workspace(n, h, w, cin)
    ws = G.workspace(nbytes)
    call("unetdc_conv3x3_dgrad_colsum", dyv.data_ptr(), dyv.stride(0), wd.data_ptr(), dx1.data_ptr(), dx1.stride(0),
         out.data_ptr(), 0, c, ws.data_ptr(), nbytes, n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    assert torch.equal(dx0.float(), dx1.float())
    ref = dx1.double()[:, :c].sum(0).cpu()
    scale = float(dx1.double()[:, :c].abs().sum(0).max())
    assert float((out.cpu().double() - ref).abs().max()) <= 2e-6 * scale
    # a column window that does not start at 0
    out2 = torch.full((16,), float("nan"), device="cuda")
    call("unetdc_conv3x3_dgrad_colsum", dyv.data_ptr(), dyv.stride(0), wd.data_ptr(), dx1.data_ptr(), dx1.stride(0),
         out2.data_ptr(), cin - 16, 16, ws.data_ptr(), nbytes, n, h, w, cin, cout, d, G.DT[dtype], G.stream())
    ref2 = dx1.double()[:, cin - 16:].sum(0).cpu()
    assert float((out2.cpu().double() - ref2).abs().max()) <= 2e-6 * float(dx1.double().abs().sum(0).max())


@pytest.mark.parametrize("case", [(8, 512, 512, 64, 64, 1), (8, 256, 256, 128, 128, 2), (8, 64, 64, 512, 512, 8),
                                  (8, 512, 512, 128, 64, 1), (8, 32, 32, 1024, 1024, 16), (8, 128, 128, 256, 512, 1)])
def test_fused_bn_backward_statistics_are_run_to_run_deterministic(case):
    """Full-size layers of the headline config (bs 8, 512x512): dgrad + fused BatchNorm-backward partial sums,
    six runs, bitwise identical output AND partial rows.  Regression test for a build whose packed-fp32
    epilogue dropped single-pixel contributions in about one workgroup out of 8192 (igemm_epilogue.h, BUILD
    NOTE) -- small-shape parity tests cannot see that."""
    import ctypes
    n, h, w, cin, cout, d = case
    P = n * h * w
    g = gen(3)
    dy = torch.randn(P, cout, generator=g).bfloat16().cuda()
    yprev = torch.randn(P, cin, generator=g).bfloat16().cuda()
    _, wd = G.pack_conv(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5), "bf16")
    sc, sh, mu, rs = (torch.randn(cin, generator=g).cuda() for _ in range(4))
    rows = _lib.load().unetdc_conv3x3_stats_rows(P, cin)
    first = None
    for it in range(6):
        dx = torch.full((P, cin), float("nan"), dtype=torch.bfloat16, device="cuda")
        parts = torch.full(((rows + 64) * 3 * cin,), float("nan"), device="cuda")
        npart = ctypes.c_int(0)
        call("unetdc_conv3x3_dgrad_bnstats", dy.data_ptr(), cout, wd.data_ptr(), dx.data_ptr(), cin, yprev.data_ptr(), cin,
             sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr(), parts.data_ptr(), parts.numel(),
             ctypes.byref(npart), n, h, w, cin, cout, d, G.DT["bf16"], G.stream())
        torch.cuda.synchronize()
        cur = (dx.view(torch.int16).clone(), parts[: npart.value * 3 * cin].view(torch.int32).clone())
        assert not torch.isnan(parts[: npart.value * 3 * cin]).any()
        if first is None:
            first = cur
        else:
            assert torch.equal(first[0], cur[0]), f"dx differs in run {it}"
            nbad = int((first[1] != cur[1]).sum())
            assert nbad == 0, f"{nbad} partial sums differ in run {it}"


@pytest.mark.parametrize("case", [("conv", 8, 64, 64, 512, 512, 1), ("conv", 8, 256, 256, 64, 128, 2), ("conv", 8, 128, 128, 256, 256, 4),
                                  ("conv", 8, 64, 64, 1024, 512, 1), ("convt", 8, 32, 32, 1024, 512, 1), ("convt", 8, 256, 256, 128, 64, 1)])
def test_weight_gradients_are_run_to_run_deterministic(case):
    """Full-size layers (bs 8): the paired tap-split weight gradients (two K ranges per workgroup meeting in LDS, fp32 slabs summed
    in a fixed order) and the tap-fused ConvTranspose2d weight gradient -- three runs, bitwise identical."""
    kind, n, h, w, cin, cout, d = case
    g = gen(5)
    lib = _lib.load()
    x = torch.randn(n * h * w, cin, generator=g).bfloat16().cuda()
    if kind == "conv":
        dy = torch.randn(n * h * w, cout, generator=g).bfloat16().cuda()
        runs = [G.conv3x3_wgrad(x, dy, n, h, w, cin, cout, d, "bf16") for _ in range(3)]
    else:
        dup = torch.randn(n * 4 * h * w, cout, generator=g).bfloat16().cuda()
        nbytes = lib.unetdc_convT2x2_wgrad_workspace(n, h, w, cin, cout, G.DT["bf16"])
        ws = G.workspace(nbytes)
        runs = []
        for _ in range(3):
            dw = torch.full((cin, cout, 2, 2), float("nan"), device="cuda")
            call("unetdc_convT2x2_wgrad", x.data_ptr(), cin, dup.data_ptr(), cout, dw.data_ptr(), ws.data_ptr(), nbytes, n, h, w,
                 cin, cout, G.DT["bf16"], G.stream())
            runs.append(dw)
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_fused_focal_dice_loss(gamma):
    """Fused HIP loss vs the reference's own numbers (golden) and vs the PyTorch formulation."""
    from tests.helpers import load_golden
    from utils import metrics_DC as M
    ops = load_golden("ops")
    p = torch.from_numpy(ops["loss_p"]).cuda().requires_grad_(True)
    t = torch.from_numpy(ops["loss_t"]).cuda()
    if gamma == 2.0:
        loss = M.focal_dice_loss(p, t, alpha=1.0, gamma=2.0, ratio=0.3)
        assert abs(loss.item() - float(ops["loss_val"])) < 1e-6
        loss.backward()
        np.testing.assert_allclose(p.grad.cpu().numpy(), ops["loss_gp"], atol=1e-7, rtol=1e-4)
    g = gen(23)
    pr = torch.rand(3, 2, 40, 56, generator=g)
    pr[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7])          # log clamps
    tg = (torch.rand(3, 2, 40, 56, generator=g) < 0.3).float()
    a = pr.clone().cuda().requires_grad_(True)
    b = pr.clone().cuda().requires_grad_(True)
    lf = M.focal_dice_loss(a, tg.cuda(), alpha=0.75, gamma=gamma, ratio=0.4)
    lt = 0.4 * M.FocalLoss(alpha=0.75, gamma=gamma)(b, tg.cuda()) + 0.6 * M.dice_loss(b, tg.cuda())
    assert abs(lf.item() - lt.item()) < 2e-6 * max(1.0, abs(lt.item()))
    (lf * 3.0).backward()
    (lt * 3.0).backward()
    fin = torch.isfinite(b.grad)
    assert torch.equal(torch.isfinite(a.grad), fin)
    assert float((a.grad[fin] - b.grad[fin]).abs().max()) < 1e-6 * float(b.grad[fin].abs().max()) + 1e-9
