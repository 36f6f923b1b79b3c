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
    """Output views (fill='nan') are surrounded by the NaN pattern of NAN_BITS; input views (fill='sentinel') by SENTINEL."""
    assert 0 <= off and off + cols <= ld
    buf = torch.empty((rows + 2 * margin) * ld, dtype=dtype, device=device)
    if fill == "nan":
        buf.view(INT_VIEW[dtype]).fill_(_signed(NAN_BITS[dtype], dtype))
    else:
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
}
ARGS = {k: tuple(v.split()) for k, v in ARGS.items()}
SHAPE_NAMES = ("n", "h", "w", "wd", "cin", "cout", "dilation", "c0", "c")
CANON = {"wd": "w"}                      # the first-layer symbols call the image width `wd` (their `w` is the weight)


def positions(sym, kinds):
    """name -> position for the arguments of `sym` that the replay reads: shapes (int), lds, dtype, pointers, workspace."""
    out = {}
    for i, (name, kind) in enumerate(zip(ARGS[sym], kinds)):
        if kind == "I" and (name in SHAPE_NAMES or name.startswith("ld") or name == "dtype"):
            out[CANON.get(name, name)] = i
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
