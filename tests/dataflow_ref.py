"""Dataflow reference of one U-Net / U-Net-DC step at the level of its storage points (CPU importable, no engine import).

The graph is restated from the module's own definition (``_UNetFamily._forward_aten_cpu``: encoder blocks, 2x2 max-pool,
bottleneck, ``upconv<l>`` then ``dec<l>(cat([up, skip]))``, 1x1 head, sigmoid) and from the Sequential layout of a block
(conv, BatchNorm, ReLU, conv, BatchNorm, ReLU), never from the HIP engine or its plan.  Every value has a name:

  forward   ``<S>.y`` raw conv output of stage S (``enc1.0`` ... ``dec1.3``), ``<S>.mean/rstd/scale/shift``,
            ``<S>.running_mean/running_var``, ``<S>.a`` activation, ``<B>.pool`` pooled copy of encoder block B,
            ``up<l>`` output of ``upconv<l>``, ``probs``, ``loss``;
  backward  ``dprobs``, ``g:<S>.a`` incoming gradient of an activation (for an encoder's second stage: the two parts
            ``g:<B>.skip`` (second half of the concat gradient) and ``g:<B>.pool``), ``g:up<l>`` (first half),
            ``<S>.dy``, ``G:<parameter>`` every parameter gradient, ``dx`` (dL/dx, NCHW);
  inputs    ``x`` (NCHW), ``target``, ``P:<state_dict key>`` parameters and running buffers as they stood at the forward.

``reference(graph, names, get, dt, mode)`` computes every asked value from its model-level SOURCES, fetched through
``get(name) -> (tensor, uncertainty or None)``: the stored value (teacher forcing: uncertainty None) or, for a value that
is never materialised, a derived one.  Each reference comes with a per-element bound derived from the fp32 operation
sequence of the kernel that produces it:

  * accumulation: ``SUM_TOL * sum |a_i b_i|`` (as in tests/test_gpu_exact.py) for every fp32 sum;
  * storage rounding of the output: not in the bound -- exact_ref.within_bound accepts the rounding of any value within
    it (either neighbour only where the reference lies within the bound of a rounding boundary);
  * BatchNorm statistics: the kernels may sum the fp32 outputs before their rounding to the stored type, the reference
    sees the stored values, so every summed term carries half an ulp of the storage type;
  * a derived (not materialised) input carries its own uncertainty into its consumer's bound.

Spatial values are NHWC ``[N, H, W, C]``; fp64 throughout.  ``dt`` is the storage dtype of the step (bfloat16 / float32),
or float64 for the unrounded chain of tests/test_dataflow_ref_cpu.py."""
import torch
import torch.nn as nn

from tests import exact_ref as X

E = X.EPS32
SUM_TOL = 4e-6                           # fp32 accumulation of any sum: |err| <= SUM_TOL * sum |terms| (~64 ulp)
_TINY = 2.0 ** -126


def unit(dt):
    """Unit roundoff of storing through dt (half an ulp, relative)."""
    return {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}.get(dt, 0.0)


def store(x, dt):
    """The stored value of x (fp64 tensor) through dt; identity for the fp64 chain."""
    return x if dt == torch.float64 else X.to_storage(x, dt).to(torch.float64)


def fp32(v, dt=torch.float32):
    """A hyper-parameter as the kernels receive it (an fp32 argument); exact for the fp64 chain."""
    return float(v) if dt == torch.float64 else float(torch.tensor(float(v), dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------- the graph
class Stage:
    def __init__(self, block, idx, level, conv, bn, src):
        self.block, self.idx, self.level, self.src = block, idx, level, src
        self.name = f"{block}.{idx}"
        self.conv_name, self.bn_name = f"{block}.{idx}", f"{block}.{idx + 1}"
        self.cin, self.cout, self.dil = conv.in_channels, conv.out_channels, conv.dilation[0]
        self.eps, self.momentum = bn.eps, (0.1 if bn.momentum is None else bn.momentum)
        self.first = src == ("x",)


class Graph:
    """The U-Net family's graph from the module: encoder blocks (named enc*) in registration order, then ``bottleneck``,
    then ``upconv<l>`` / ``dec<l>`` pairs, then ``out_conv``.  src of a stage: ("x",), ("act", S), ("pool", B) or
    ("cat", "up<l>", "<enc>.3")."""

    def __init__(self, model):
        kids = dict(model.named_children())
        enc = [k for k in kids if k.startswith("enc")]
        decs = [k for k in kids if k.startswith("dec")]
        self.stages, self.ups = [], {}
        prev = ("x",)
        for lvl, b in enumerate(enc):                     # h = enc(h); skip; h = max_pool2d(h, 2)
            self._block(kids, b, lvl, prev)
            prev = ("pool", b)
        self._block(kids, "bottleneck", len(enc), prev)
        h = "bottleneck.3"
        for b in decs:                                    # up = upconv<l>(h); h = dec<l>(cat([up, skips[l - 1]]))
            lvl = int(b[3:])
            up = kids[f"upconv{lvl}"]
            assert isinstance(up, nn.ConvTranspose2d) and up.kernel_size == (2, 2) and up.stride == (2, 2)
            self.ups[f"up{lvl}"] = dict(mod=f"upconv{lvl}", src=h, cin=up.in_channels, cout=up.out_channels, level=lvl - 1)
            self._block(kids, b, lvl - 1, ("cat", f"up{lvl}", f"{enc[lvl - 1]}.3"))
            h = f"{b}.3"
        self.last = h
        self.encoders = enc
        self.by_name = {s.name: s for s in self.stages}
        head = kids["out_conv"]
        assert head.kernel_size == (1, 1)
        self.oc = head.out_channels

    def _block(self, kids, b, lvl, src):
        seq = kids[b]
        assert isinstance(seq[0], nn.Conv2d) and isinstance(seq[1], nn.BatchNorm2d) and isinstance(seq[2], nn.ReLU)
        assert isinstance(seq[3], nn.Conv2d) and isinstance(seq[4], nn.BatchNorm2d) and isinstance(seq[5], nn.ReLU)
        self.stages.append(Stage(b, 0, lvl, seq[0], seq[1], src))
        self.stages.append(Stage(b, 3, lvl, seq[3], seq[4], ("act", f"{b}.0")))

    # ------------------------------------------------------------------ value lists
    def consumer_of_input(self, st):
        """Gradient value names the input-gradient of stage st produces."""
        k = st.src[0]
        if k == "x":
            return ["dx"]
        if k == "act":
            return [f"g:{st.src[1]}.a"]
        if k == "pool":
            return [f"g:{st.src[1]}.pool"]
        return [f"g:{st.src[1]}", f"g:{st.src[2][:-2]}.skip"]

    def forward_values(self, mode):
        out = []
        for st in self.stages:
            for u, d in self.ups.items():
                if st.src[0] == "cat" and st.src[1] == u:
                    out.append(u)
            if mode == "eval":
                out += [f"{st.name}.scale", f"{st.name}.shift", f"{st.name}.a"]
            else:
                out += [f"{st.name}.y", f"{st.name}.mean", f"{st.name}.rstd", f"{st.name}.scale", f"{st.name}.shift"]
                if mode == "train":
                    out += [f"{st.name}.running_mean", f"{st.name}.running_var"]
                out.append(f"{st.name}.a")
            if st.idx == 3 and st.block in self.encoders:
                out.append(f"{st.block}.pool")
        return out + ["probs"]

    def backward_values(self, need_dx):
        out = ["G:out_conv.weight", "G:out_conv.bias", f"g:{self.last}.a"]
        for st in reversed(self.stages):
            out += [f"{st.name}.dy", f"G:{st.bn_name}.weight", f"G:{st.bn_name}.bias", f"G:{st.conv_name}.bias",
                    f"G:{st.conv_name}.weight"]
            if not st.first or need_dx:
                out += self.consumer_of_input(st)
            if st.src[0] == "cat":
                u = self.ups[st.src[1]]
                out += [f"G:{u['mod']}.bias", f"G:{u['mod']}.weight", f"g:{u['src']}.a"]
        return out


# ---------------------------------------------------------------------------------------------------- helpers
def nhwc(t, n, h, w):
    return t.reshape(n, h, w, -1)


def derive_act(y, scale, shift, dt):
    """relu(fmaf(y, scale, shift)) rounded through dt, as every normalise-on-load kernel computes it (fp64 product and sum are
    exact for a bf16 / fp32 y and fp32 scale / shift; one rounding to fp32, the ReLU, the storage rounding)."""
    v = y.to(torch.float64) * scale.to(y.device, torch.float64) + shift.to(y.device, torch.float64)
    if dt == torch.float64:
        return torch.relu(v)
    return store(torch.relu(v.to(torch.float32).to(torch.float64)), dt)


def _interval_bound(ref, lo, hi):
    return torch.maximum((ref - lo).abs(), (hi - ref).abs())


def _mul(alo, ahi, blo, bhi):
    c = torch.stack([alo * blo, alo * bhi, ahi * blo, ahi * bhi])
    return c.amin(0), c.amax(0)


def _weight(get, name, dt, master=False):
    """A conv weight as the kernel reads it: the fp32 master (first layer, head) or its packed image in the compute type."""
    w = get(name)[0].to(torch.float64)
    return w if master else store(w, dt)


def _input(g, st, get, n, h, w):
    """The stage's convolution input [N, h, w, Cin] (fp64) and its uncertainty (None: exact)."""
    k = st.src[0]
    if k == "x":
        return get("x")[0].to(torch.float64).permute(0, 2, 3, 1), None
    if k == "act":
        return nhwc(get(f"{st.src[1]}.a")[0], n, h, w).to(torch.float64), None
    if k == "pool":
        return nhwc(get(f"{st.src[1]}.pool")[0], n, h, w).to(torch.float64), None
    up, skip = nhwc(get(st.src[1])[0], n, h, w), nhwc(get(f"{st.src[2]}.a")[0], n, h, w)
    return torch.cat([up, skip], dim=-1).to(torch.float64), None


def stats_ref(y, gamma, beta, eps, dt):
    """nn.BatchNorm2d batch statistics of the stored y [P, C] under the bound of the kernels' fp32 partial sums of the
    unrounded outputs: sum and sum of squares each off by (SUM_TOL + storage roundoff) of their absolute terms."""
    M = y.shape[0]
    u = unit(dt)
    s, q, sa = y.sum(0), (y * y).sum(0), y.abs().sum(0)
    ds, dq = (SUM_TOL + u) * sa, (SUM_TOL + 2.01 * u) * q
    eps = fp32(eps, dt)
    mean, var = s / M, (q / M - (s / M) ** 2).clamp_min(0.0)
    mlo, mhi = (s - ds) / M, (s + ds) / M
    msq_hi = torch.maximum(mlo * mlo, mhi * mhi)
    msq_lo = torch.where((mlo <= 0) & (mhi >= 0), torch.zeros_like(mlo), torch.minimum(mlo * mlo, mhi * mhi))
    vlo, vhi = ((q - dq) / M - msq_hi).clamp_min(0.0), (q + dq) / M - msq_lo
    rstd = 1.0 / torch.sqrt(var + eps)
    rlo, rhi = 1.0 / torch.sqrt(vhi + eps), 1.0 / torch.sqrt(vlo + eps)
    g, b = gamma.to(torch.float64), beta.to(torch.float64)
    scale = g * rstd
    slo, shi = _mul(g, g, rlo, rhi)
    shift = b - mean * scale
    plo, phi = _mul(mlo, mhi, slo, shi)
    out = dict(mean=(mean, _interval_bound(mean, mlo, mhi) + 4 * E * mean.abs()),
               rstd=(rstd, _interval_bound(rstd, rlo, rhi) + 4 * E * rstd),
               scale=(scale, _interval_bound(scale, slo, shi) + 4 * E * scale.abs()),
               shift=(shift, _interval_bound(shift, b - phi, b - plo) + 4 * E * (shift.abs() + (mean * scale).abs())),
               var=(var, _interval_bound(var, vlo, vhi)))
    return out


def running_ref(stats, rm, rv, M, momentum, dt):
    m = fp32(momentum, dt)
    mean, dmean = stats["mean"]
    var, dvar = stats["var"]
    rm, rv = rm.to(torch.float64), rv.to(torch.float64)
    k = M / (M - 1.0) if M > 1 else 1.0
    new_m = (1 - m) * rm + m * mean
    new_v = (1 - m) * rv + m * var * k
    return dict(running_mean=(new_m, 4 * E * ((1 - m) * rm.abs() + m * mean.abs()) + m * dmean + _TINY),
                running_var=(new_v, 4 * E * ((1 - m) * rv.abs() + m * var * k) + m * k * dvar + _TINY))


def head_dz(dprobs, probs):
    """dz = dprobs * p * (1 - p) [N, OC, H, W] -> [P, OC] and its fp32 bound (three roundings)."""
    oc = probs.shape[1]
    dz = X.head_dz(dprobs, probs).permute(0, 2, 3, 1).reshape(-1, oc)
    return dz, 4 * E * dz.abs()


# ---------------------------------------------------------------------------------------------------- references
def reference(g, names, get, dt, mode, dims, need_dx=False):
    """{name: (ref, bound)} for the asked value names (those produced by one call).  dims = (N, H, W) of the input.
    get(name) -> (tensor, uncertainty or None)."""
    N, H, W = dims
    res = {}
    for name in names:
        if name in res:
            continue
        if name in ("loss", "dprobs"):
            res.update(_loss(get, N))
        elif name == "probs":
            res.update(_head_fwd(g, get, dt, N, H, W))
        elif name in ("G:out_conv.weight", "G:out_conv.bias", f"g:{g.last}.a"):
            res.update(_head_bwd(g, get, dt, N, H, W))
        elif name in g.ups:
            res.update(_up_fwd(g, name, get, N, H, W))
        elif (name.startswith("G:upconv") and name.endswith(".weight")) or (name.startswith("g:") and name.endswith(".3.a") and name[2:-2] != g.last
                                             and any(u["src"] == name[2:-2] for u in g.ups.values())):
            res.update(_up_bwd(g, name, get, dt, N, H, W))
        elif name.endswith(".pool") and not name.startswith("g:"):
            st = g.by_name[f"{name[:-5]}.3"]
            a = nhwc(get(f"{st.name}.a")[0], N, H >> st.level, W >> st.level).to(torch.float64)
            r = X.maxpool2(a)
            res[name] = (r, torch.zeros_like(r))
        else:
            st = next((s for s in g.stages if name in _stage_value_names(g, s)), None)
            if st is None:
                raise KeyError(name)
            res.update(_stage(g, st, name, get, dt, mode, N, H, W))
    return {k: v for k, v in res.items() if k in names}


def _fwd_names(st):
    S = st.name
    return {f"{S}.{k}" for k in ("y", "mean", "rstd", "scale", "shift", "running_mean", "running_var", "a")}


def _stage_value_names(g, st):
    S = st.name
    bwd = {f"{S}.dy", f"G:{st.bn_name}.weight", f"G:{st.bn_name}.bias", f"G:{st.conv_name}.bias", f"G:{st.conv_name}.weight"}
    if st.src[0] == "cat":
        bwd.add(f"G:{g.ups[st.src[1]]['mod']}.bias")
    return _fwd_names(st) | bwd | set(g.consumer_of_input(st))


def _stage(g, st, name, get, dt, mode, N, H, W):
    S = st.name
    h, w = H >> st.level, W >> st.level
    P = N * h * w
    gamma, beta = get(f"P:{st.bn_name}.weight")[0], get(f"P:{st.bn_name}.bias")[0]
    out = {}
    if name == f"{S}.y":
        x, _ = _input(g, st, get, N, h, w)
        wt = _weight(get, f"P:{st.conv_name}.weight", dt, master=st.first)
        b = get(f"P:{st.conv_name}.bias")[0].to(x.device, torch.float64)
        acc = X.conv3x3_fwd(x, wt, st.dil)
        bnd = SUM_TOL * X.conv3x3_fwd(x.abs(), wt.abs(), st.dil) + E * (acc.abs() + b.abs()) + _TINY
        out[name] = (acc + b, bnd)
    elif name in (f"{S}.mean", f"{S}.rstd", f"{S}.scale", f"{S}.shift", f"{S}.running_mean", f"{S}.running_var"):
        if mode == "train":
            y = get(f"{S}.y")[0].reshape(P, -1).to(torch.float64)
            stt = stats_ref(y, gamma.to(y.device), beta.to(y.device), st.eps, dt)
            for k in ("mean", "rstd", "scale", "shift"):
                out[f"{S}.{k}"] = stt[k]
            rm, rv = get(f"P:{st.bn_name}.running_mean")[0], get(f"P:{st.bn_name}.running_var")[0]
            for k, v in running_ref(stt, rm.to(y.device), rv.to(y.device), P, st.momentum, dt).items():
                out[f"{S}.{k}"] = v
        else:
            rm, rv = get(f"P:{st.bn_name}.running_mean")[0], get(f"P:{st.bn_name}.running_var")[0]
            eps = fp32(st.eps, dt)
            if mode == "frozen":
                r = X.bn_frozen_affine(gamma, beta, rm, rv, eps)
                out[f"{S}.mean"] = (r["mean"], torch.zeros_like(r["mean"]))
                out[f"{S}.rstd"] = (r["rstd"], 8 * E * r["rstd"])
                out[f"{S}.scale"] = (r["scale"], 10 * E * r["scale"].abs())
                out[f"{S}.shift"] = (r["shift"], 2 * E * r["shift"].abs() + 14 * E * (r["mean"] * r["scale"]).abs())
            else:
                cb = get(f"P:{st.conv_name}.bias")[0]
                r = X.bn_eval_affine(gamma, beta, rm, rv, eps, cb)
                d = cb.to(torch.float64) - rm.to(torch.float64)
                out[f"{S}.scale"] = (r["scale"], 8 * E * r["scale"].abs())
                out[f"{S}.shift"] = (r["shift"], 2 * E * r["shift"].abs() + 12 * E * (d * r["scale"]).abs())
    elif name == f"{S}.a":
        sc, sh = get(f"{S}.scale")[0].to(torch.float64), get(f"{S}.shift")[0].to(torch.float64)
        if mode == "eval":
            x, _ = _input(g, st, get, N, h, w)
            wt = _weight(get, f"P:{st.conv_name}.weight", dt, master=st.first)
            acc = X.conv3x3_fwd(x, wt, st.dil)
            nrm = acc * sc.to(acc.device) + sh.to(acc.device)
            bnd = SUM_TOL * X.conv3x3_fwd(x.abs(), wt.abs(), st.dil) * sc.abs().to(acc.device) + E * nrm.abs() + _TINY
        else:
            y = get(f"{S}.y")[0].to(torch.float64)
            nrm = nhwc(y, N, h, w) * sc.to(y.device) + sh.to(y.device)
            bnd = E * nrm.abs() + _TINY
        out[name] = (torch.relu(nrm), torch.where(nrm > 0, bnd, torch.zeros_like(bnd)) if dt == torch.float64 else bnd)
    elif name in (f"{S}.dy", f"G:{st.bn_name}.weight", f"G:{st.bn_name}.bias", f"G:{st.conv_name}.bias"):
        out.update(_bn_bwd(g, st, get, dt, mode, N, h, w))
    elif name == f"G:{st.conv_name}.weight":
        x, _ = _input(g, st, get, N, h, w)
        dy, udy = get(f"{S}.dy")
        dy = nhwc(dy, N, h, w).to(torch.float64)
        dw = X.conv3x3_wgrad(x, dy, st.dil)
        bnd = SUM_TOL * X.conv3x3_wgrad(x.abs(), dy.abs(), st.dil)
        if udy is not None:
            bnd = bnd + X.conv3x3_wgrad(x.abs(), nhwc(udy, N, h, w), st.dil)
        out[name] = (dw, bnd)
    else:                                                   # the input gradient: dgrad of dy through the layer's weights
        dy = nhwc(get(f"{S}.dy")[0], N, h, w).to(torch.float64)
        wt = _weight(get, f"P:{st.conv_name}.weight", dt, master=st.first)
        dx = X.conv3x3_dgrad(dy, wt, st.dil)
        bnd = SUM_TOL * X.conv3x3_dgrad(dy.abs(), wt.abs(), st.dil) + _TINY
        names = g.consumer_of_input(st)
        if st.src[0] == "x":
            out["dx"] = (dx.permute(0, 3, 1, 2), bnd.permute(0, 3, 1, 2))
        elif st.src[0] == "cat":
            c = g.ups[st.src[1]]["cout"]
            out[names[0]] = (dx[..., :c], bnd[..., :c])
            out[names[1]] = (dx[..., c:], bnd[..., c:])
            # the up-convolution's bias gradient: the column sums of the first half as the dgrad computes it (fp32 values,
            # before or after their storage rounding)
            gu = dx[..., :c].reshape(-1, c)
            u = g.ups[st.src[1]]
            out[f"G:{u['mod']}.bias"] = (gu.sum(0), (SUM_TOL + unit(dt)) * gu.abs().sum(0)
                                         + (bnd[..., :c].reshape(-1, c)).sum(0) + _TINY)
        else:
            out[names[0]] = (dx, bnd)
    return out


def _bn_bwd(g, st, get, dt, mode, N, h, w):
    """Backward of y -> BatchNorm -> ReLU (-> skip and 2x2 max-pool): dy, dgamma, dbeta, the conv bias gradient."""
    S = st.name
    P = N * h * w
    y = nhwc(get(f"{S}.y")[0], N, h, w).to(torch.float64)
    dev = y.device
    sc, sh, mu, rs = (get(f"{S}.{k}")[0].to(dev, torch.float64) for k in ("scale", "shift", "mean", "rstd"))
    gamma = get(f"P:{st.bn_name}.weight")[0].to(dev, torch.float64)
    nrm = y * sc + sh
    ug = None
    if st.idx == 3 and st.block in g.encoders:
        skip = nhwc(get(f"g:{st.block}.skip")[0], N, h, w).to(torch.float64)
        dpool = nhwc(get(f"g:{st.block}.pool")[0], N, h // 2, w // 2).to(torch.float64)
        a = nhwc(get(f"{S}.a")[0], N, h, w).to(torch.float64)      # the pool's arg-max: first maximum of the stored activation
        gin = skip + X.pool_scatter(dpool, X.pool_argmax(a), h, w)
    else:
        gv, ug = get(f"g:{S}.a")
        gin = nhwc(gv, N, h, w).to(torch.float64)
        ug = None if ug is None else nhwc(ug, N, h, w)
    gate = nrm > 0
    gh = torch.where(gate, gin, torch.zeros_like(gin))
    ugh = None if ug is None else torch.where(gate, ug, torch.zeros_like(ug))
    xh = (y - mu) * rs
    c = y.shape[-1]
    f = lambda t: t.reshape(-1, c).sum(0)                   # noqa: E731
    s1, s2, s3 = f(gh), f(gh * xh), f(xh)
    d1, d2, d3 = SUM_TOL * f(gh.abs()), SUM_TOL * f((gh * xh).abs()), SUM_TOL * f(xh.abs())
    if ugh is not None:
        d1, d2 = d1 + f(ugh), d2 + f(ugh * xh.abs())
    k1 = gamma * rs
    frozen = mode == "frozen"
    if frozen:
        k2, k3, dk2, dk3 = (torch.zeros_like(k1),) * 4
        dbias, ddbias = k1 * s1, k1.abs() * d1 + 2 * E * (k1 * s1).abs()
    else:
        k2, k3 = k1 * s1 / P, k1 * s2 / P
        dk2, dk3 = k1.abs() * d1 / P + 2 * E * k2.abs(), k1.abs() * d2 / P + 2 * E * k3.abs()
        dbias = -k3 * s3
        ddbias = k3.abs() * d3 + dk3 * s3.abs() + 2 * E * dbias.abs()
    dy = k1 * gh - k2 - k3 * xh
    bnd = 4 * E * ((k1 * gh).abs() + k2.abs() + (k3 * xh).abs()) + dk2 + dk3 * xh.abs() + _TINY
    if ugh is not None:
        bnd = bnd + k1.abs() * ugh
    return {f"{S}.dy": (dy, bnd), f"G:{st.bn_name}.weight": (s2, d2 + E * s2.abs() + _TINY),
            f"G:{st.bn_name}.bias": (s1, d1 + E * s1.abs() + _TINY), f"G:{st.conv_name}.bias": (dbias, ddbias + _TINY)}


def _up_fwd(g, name, get, N, H, W):
    u = g.ups[name]
    lvl = u["level"] + 1
    h, w = H >> lvl, W >> lvl
    x = nhwc(get(f"{u['src']}.a")[0], N, h, w).to(torch.float64)
    dt = get(f"{u['src']}.a")[0].dtype
    wt = _weight(get, f"P:{u['mod']}.weight", dt)
    b = get(f"P:{u['mod']}.bias")[0].to(x.device, torch.float64)
    acc = X.convT2x2_fwd(x, wt)
    return {name: (acc + b, SUM_TOL * X.convT2x2_fwd(x.abs(), wt.abs()) + E * (acc.abs() + b.abs()) + _TINY)}


def _up_bwd(g, name, get, dt, N, H, W):
    if name.startswith("G:upconv"):
        lvl = name[len("G:upconv"):].split(".")[0]
    else:
        lvl = next(k[2:] for k, u in g.ups.items() if u["src"] == name[2:-2])
    u = g.ups[f"up{lvl}"]
    h, w = H >> (u["level"] + 1), W >> (u["level"] + 1)
    dup = nhwc(get(f"g:up{lvl}")[0], N, 2 * h, 2 * w).to(torch.float64)
    out = {}
    if name.endswith(".weight"):
        x = nhwc(get(f"{u['src']}.a")[0], N, h, w).to(torch.float64)
        out[name] = (X.convT2x2_wgrad(x, dup), SUM_TOL * X.convT2x2_wgrad(x.abs(), dup.abs()) + _TINY)
    else:
        wt = _weight(get, f"P:{u['mod']}.weight", dt)
        out[name] = (X.convT2x2_dgrad(dup, wt), SUM_TOL * X.convT2x2_dgrad(dup.abs(), wt.abs()) + _TINY)
    return out


def _head_act(g, get, dt, N, H, W):
    a, ua = get(f"{g.last}.a")
    return nhwc(a, N, H, W).reshape(N * H * W, -1).to(torch.float64), ua


def _head_fwd(g, get, dt, N, H, W):
    a, _ = _head_act(g, get, dt, N, H, W)
    wt, b = get("P:out_conv.weight")[0], get("P:out_conv.bias")[0]
    wt = wt.reshape(wt.shape[0], -1)
    z, p = X.head_fwd(a, wt, b, N, H, W)
    c = a.shape[1]
    oc = wt.shape[0]
    dz = (c // 2 + 8) * E * (a.abs() @ wt.abs().to(a).t()).view(N, H, W, oc).permute(0, 3, 1, 2) + E * z.abs()
    return {"probs": (p, p * (1 - p) * (dz + 8 * E) + 4 * E * p + _TINY)}


def _head_bwd(g, get, dt, N, H, W):
    a, _ = _head_act(g, get, dt, N, H, W)
    dprobs, probs = get("dprobs")[0], get("probs")[0]
    wt = get("P:out_conv.weight")[0]
    oc = wt.shape[0]
    wt = wt.reshape(oc, -1).to(a)
    dz, udz = head_dz(dprobs.to(a.device), probs.to(a.device))
    da = dz @ wt
    dab = (dz.abs() @ wt.abs()) * 4 * E + _TINY
    return {"G:out_conv.weight": ((dz.t() @ a).view(oc, -1, 1, 1), ((SUM_TOL + 4 * E) * (dz.abs().t() @ a.abs())).view(oc, -1, 1, 1)
                                  + _TINY),
            "G:out_conv.bias": (dz.sum(0), (SUM_TOL + 4 * E) * dz.abs().sum(0) + _TINY),
            f"g:{g.last}.a": (da.view(N, H, W, -1), dab.view(N, H, W, -1))}


LOSS_ARGS = dict(alpha=1.0, gamma=2.0, ratio=0.3, smooth=1e-7)     # utils.metrics_DC.focal_dice_loss defaults (fp32 values)


def loss_nsum(hw):
    """Longest chain of fp32 additions behind one per-map partial sum of the loss kernel (tests/test_gpu_exact_norm.py)."""
    import math
    nb = min(128, max(1, math.ceil(hw / 2048)))
    return math.ceil(hw / (nb * 256)) + 8


def _loss(get, N):
    p, t = get("probs")[0], get("target")[0]
    nimg, hw = p.shape[0] * p.shape[1], p.shape[2] * p.shape[3]
    p2, t2 = p.reshape(nimg, hw).to(torch.float64), t.reshape(nimg, hw).to(p.device, torch.float64)
    a = {k: fp32(v) for k, v in LOSS_ARGS.items()}
    (llo, lhi), (dlo, dhi) = X.focal_dice_bounds(p2, t2, a["alpha"], a["gamma"], a["ratio"], a["smooth"], 1.0, loss_nsum(hw))
    return {"loss": ((llo + lhi) / 2, (lhi - llo) / 2),
            "dprobs": (((dlo + dhi) / 2).view(p.shape), ((dhi - dlo) / 2).view(p.shape))}


def loss_exact(p, t):
    """The fp64 loss and d loss / d probs of the graph's criterion with its exact hyper-parameters (no rounding)."""
    nimg, hw = p.shape[0] * p.shape[1], p.shape[2] * p.shape[3]
    r = X.focal_dice(p.reshape(nimg, hw), t.reshape(nimg, hw), **LOSS_ARGS)
    return r["loss"], r["dp"].view(p.shape)


# ---------------------------------------------------------------------------------------------------- derived values
def derive(g, name, get, dt, mode, dims):
    """A value the HIP path may legitimately never store, from its sources: (value, uncertainty or None).
      * ``<S>.a`` of a training-path forward: relu(fmaf(y, scale, shift)) rounded through dt -- exactly what the
        normalise-on-load kernels compute (conv3x3_fwd_bnin / wgrad_bnin, head_fwd_bn);
      * ``g:<last>.a`` under the fused head: dz * w per pixel, recomputed by the BatchNorm backward of the last stage;
      * ``enc1.0.dy`` under the first-layer weight gradient that applies the BatchNorm backward on load."""
    N, H, W = dims
    if name.endswith(".a") and not name.startswith("g:"):
        st = g.by_name[name[:-2]]
        h, w = H >> st.level, W >> st.level
        y = nhwc(get(f"{st.name}.y")[0], N, h, w)
        return derive_act(y, get(f"{st.name}.scale")[0], get(f"{st.name}.shift")[0], dt), None
    if name == f"g:{g.last}.a":
        v, b = reference(g, [name], get, dt, mode, dims)[name]
        return v, b + unit(dt) * (v.abs() + b)
    if name.endswith(".dy"):
        v, b = reference(g, [name], get, dt, mode, dims)[name]
        return v, b + unit(dt) * (v.abs() + b)
    raise KeyError(f"{name} is not a derivable value")
