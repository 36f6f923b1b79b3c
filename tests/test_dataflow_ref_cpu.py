"""CPU tests of tests/dataflow_ref.py: the graph restatement chained in fp64 without storage rounding reproduces the module's
own fp64 CPU forward (``_forward_aten_cpu``), loss, every parameter's autograd gradient and dL/dx; and the bound helpers
reject a value one ulp outside the bound and a tie broken against the kernels' rule."""
import pytest
import torch

from tests import dataflow_ref as R
from tests import exact_ref as X

F64 = torch.float64


def chain(model, x, t, need_dx=True):
    """Every value of one training step, each computed by dataflow_ref from the chain's own earlier values."""
    g = R.Graph(model)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    vals = {"x": x, "target": t}
    vals.update({f"P:{k}": v for k, v in sd.items()})

    def get(name):
        return vals[name], None

    dims = (x.shape[0], x.shape[2], x.shape[3])
    names = g.forward_values("train") + ["loss", "dprobs"] + g.backward_values(need_dx)
    for name in names:
        if name == "loss":
            vals["loss"], vals["dprobs"] = R.loss_exact(vals["probs"], t)
        if name not in vals:
            vals.update({k: v for k, (v, _) in R.reference(g, [name], get, F64, "train", dims).items()})
    return g, vals


def close(got, exp, what, tol=1e-10, floor=0.0):
    got, exp = got.to(F64).reshape(exp.shape), exp.to(F64)
    err = float((got - exp).abs().max())
    scale = max(float(exp.abs().max()), floor)
    assert err <= tol * max(scale, 1e-300), f"{what}: max |err| {err:.3e} vs max |ref| {scale:.3e}"


# the last three: non-square maps with odd pooled sizes (45- and 120-pixel bottlenecks) and a two-output-channel head, the
# geometries tests/test_gpu_dataflow.py runs off the production shape
@pytest.mark.parametrize("arch,shape", [("unetdc", (2, 1, 32, 32)), ("unetdc", (1, 3, 64, 64)), ("unet", (2, 1, 32, 32)),
                                        ("unet", (1, 3, 64, 64)), ("unetdc", (3, 1, 48, 80)), ("unetdc", (2, 3, 96, 160)),
                                        ("unetdc2", (2, 1, 32, 48))])
def test_fp64_chain_reproduces_the_module(arch, shape):
    from models.model import UNet
    from models.model_2 import UNetDC
    from utils.metrics_DC import focal_dice_loss
    torch.manual_seed(3)
    n, c, h, w = shape
    oc = 2 if arch == "unetdc2" else 1
    model = (UNet if arch == "unet" else UNetDC)(c, oc).double().train()
    gen = torch.Generator().manual_seed(4)
    x = torch.rand(shape, generator=gen, dtype=F64)
    t = (torch.rand(n, oc, h, w, generator=gen) < 0.3).to(F64)
    g, vals = chain(model, x, t)
    # the module, fp64, autograd
    xr = x.clone().requires_grad_()
    p = model._forward_aten_cpu(xr)
    loss = focal_dice_loss(p, t, alpha=1.0, gamma=2.0, ratio=0.3)
    loss.backward()
    close(vals["probs"], p.detach(), "probs")
    close(vals["loss"], loss.detach(), "loss")
    close(vals["dx"], xr.grad, "dL/dx")
    for k, prm in model.named_parameters():
        # a conv bias in front of a BatchNorm has a gradient that is zero up to rounding: scaled by its BatchNorm's dbeta
        st = g.by_name.get(k[:-len(".bias")]) if k.endswith(".bias") else None
        floor = float(prm.grad.new_tensor(0).abs()) if st is None else float(getattr(model, st.block)[st.idx + 1].bias.grad.abs().max())
        close(vals[f"G:{k}"], prm.grad, f"grad {k}", floor=floor)
    # the running statistics the training forward left in the module
    for st in g.stages:
        bn = getattr(model, st.block)[st.idx + 1]
        close(vals[f"{st.name}.running_mean"], bn.running_mean, f"{st.name} running_mean")
        close(vals[f"{st.name}.running_var"], bn.running_var, f"{st.name} running_var")
    # every value of the graph was produced once, and the value lists name distinct values
    names = g.forward_values("train") + g.backward_values(True)
    assert len(names) == len(set(names))
    assert len([k for k in vals if k.startswith("G:")]) == len(list(model.parameters()))


def test_graph_follows_the_module_definition():
    from models.model_2 import UNetDC
    g = R.Graph(UNetDC(1, 1))
    assert [s.name for s in g.stages][:4] == ["enc1.0", "enc1.3", "enc2.0", "enc2.3"]
    assert g.by_name["dec1.0"].src == ("cat", "up1", "enc1.3")           # torch.cat([up, skip], 1): up first
    assert g.by_name["enc2.0"].src == ("pool", "enc1")
    assert g.by_name["bottleneck.0"].src == ("pool", "enc4")
    assert g.ups["up4"]["src"] == "bottleneck.3" and g.ups["up1"]["src"] == "dec2.3"
    assert [g.by_name[f"enc{i}.0"].dil for i in (1, 2, 3, 4)] == [1, 2, 4, 8] and g.by_name["bottleneck.3"].dil == 16
    assert g.last == "dec1.3"


def test_within_bound_rejects_one_ulp_beyond_the_bound():
    ref = torch.tensor([1.0, -3.0, 0.75], dtype=F64)
    bound = torch.tensor([2.0 ** -10, 2.0 ** -9, 0.0], dtype=F64)
    ok = X.to_storage(ref, torch.bfloat16)
    assert not X.within_bound(ok, ref, bound, torch.bfloat16).any()
    # the farthest stored value the bound admits, then one bf16 ulp beyond it, on both sides
    for sign in (1, -1):
        edge = X.to_storage(ref + sign * bound, torch.bfloat16).to(F64)
        assert not X.within_bound(edge, ref, bound, torch.bfloat16).any()
        ulp = 2.0 ** (torch.floor(torch.log2(edge.abs())) - 7)
        beyond = edge + sign * ulp
        assert X.within_bound(beyond, ref, bound, torch.bfloat16).all()


def test_within_bound_either_neighbour_only_near_a_rounding_boundary():
    # 1 + 2^-8 is the midpoint between the bf16 values 1 and 1 + 2^-7: within a bound it may be stored as either
    ref = torch.tensor([1.0 + 2.0 ** -8], dtype=F64)
    assert not X.within_bound(torch.tensor([1.0 + 2.0 ** -7]), ref, 2.0 ** -12, torch.bfloat16).any()
    assert not X.within_bound(torch.tensor([1.0]), ref, 2.0 ** -12, torch.bfloat16).any()
    # away from the boundary only the rounding of the reference is accepted
    ref = torch.tensor([1.0 + 2.0 ** -7 + 2.0 ** -10], dtype=F64)
    assert X.within_bound(torch.tensor([1.0]), ref, 2.0 ** -12, torch.bfloat16).all()


def _one_window(a_vals, y_vals, gpool):
    """An encoder's second stage on one 2x2 window, one channel: stored activation a, raw y (scale 1, shift 0)."""
    from models.model_2 import UNetDC
    g = R.Graph(UNetDC(1, 1))
    st = g.by_name["enc1.3"]
    vals = {"enc1.3.y": torch.tensor(y_vals, dtype=F64).view(4, 1), "enc1.3.a": torch.tensor(a_vals, dtype=F64).view(4, 1),
            "enc1.3.scale": torch.ones(1, dtype=F64), "enc1.3.shift": torch.zeros(1, dtype=F64),
            "enc1.3.mean": torch.zeros(1, dtype=F64), "enc1.3.rstd": torch.ones(1, dtype=F64),
            "P:enc1.4.weight": torch.ones(1, dtype=F64), "g:enc1.skip": torch.zeros(4, 1, dtype=F64),
            "g:enc1.pool": torch.tensor([[gpool]], dtype=F64)}
    return R._bn_bwd(g, st, lambda k: (vals[k], None), torch.float32, "frozen", 1, 2, 2)["enc1.3.dy"]


def test_pool_tie_goes_to_the_first_maximum_only():
    dy, bnd = _one_window([0.5, 0.5, 0.25, 0.5], [0.5, 0.5, 0.25, 0.5], 1.0)
    assert dy.view(-1).tolist() == [1.0, 0.0, 0.0, 0.0]
    assert not X.within_bound(torch.tensor([1.0, 0.0, 0.0, 0.0]), dy.view(-1), bnd.view(-1), torch.float32).any()
    # the same tie broken the other way (gradient to the second maximum) is an error
    bad = X.within_bound(torch.tensor([0.0, 1.0, 0.0, 0.0]), dy.view(-1), bnd.view(-1), torch.float32)
    assert bad.tolist() == [True, True, False, False]


def test_relu_gate_is_closed_at_zero():
    # scale * y + shift == 0 exactly: the ReLU passes no gradient (kernels: fmaf(y, scale, shift) > 0)
    dy, bnd = _one_window([0.0, 0.0, 0.0, 0.0], [0.0, -1.0, -1.0, -1.0], 1.0)
    assert dy.view(-1).tolist() == [0.0, 0.0, 0.0, 0.0]
    assert X.within_bound(torch.tensor([1.0, 0.0, 0.0, 0.0]), dy.view(-1), bnd.view(-1), torch.float32)[0]


def test_derived_activation_rounds_once_to_fp32_then_to_storage():
    # y * scale + shift lands just above a bf16 midpoint only in fp64: the fp32 rounding in between decides
    y = torch.tensor([[1.0]], dtype=F64)
    sh = torch.tensor([2.0 ** -8 + 2.0 ** -30], dtype=F64)                # fp32 rounds the 2^-30 away: a tie, to even
    a = R.derive_act(y, torch.ones(1, dtype=F64), sh, torch.bfloat16)
    assert a.item() == 1.0
    assert R.derive_act(y, torch.ones(1, dtype=F64), -torch.ones(1, dtype=F64) * 2, torch.bfloat16).item() == 0.0


# ---------------------------------------------------------------------------------------------------- bounds at small counts
def _f32_bn_stage(y, gamma, beta, rm, rv, eps, mom, gin):
    """One BatchNorm + ReLU stage forward and backward in plain fp32 torch from the stored inputs, every sum taken in an order
    of its own (pixels reversed, pairwise over two interleaved halves) -- neither the reference's nor the kernels'."""
    f = torch.float32
    y32, g32 = y.to(f), gin.to(f)
    M = y32.shape[0]

    def colsum(t):
        t = t.flip(0)
        return t[0::2].sum(0) + t[1::2].sum(0)
    s, q = colsum(y32), colsum(y32 * y32)
    m = torch.tensor(float(M), dtype=f)
    mean = s / m
    var = (q / m - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + torch.tensor(eps, dtype=f))
    scale = gamma.to(f) * rstd
    shift = beta.to(f) - mean * scale
    mo = torch.tensor(mom, dtype=f)
    out = {"mean": mean, "rstd": rstd, "scale": scale, "shift": shift,
           "running_mean": (1 - mo) * rm.to(f) + mo * mean, "running_var": (1 - mo) * rv.to(f) + mo * (var * (m / (m - 1)))}
    return out, y32, g32, colsum, m


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
# (no encoder's second stage here: its gradient arrives through the max-pool in two parts, which the operator-level pooled
# cases of tests/test_gpu_exact_norm.py cover; every stage below takes one incoming gradient g:<S>.a)
@pytest.mark.parametrize("dims,stage", [((3, 48, 80), "bottleneck.3"), ((2, 96, 160), "bottleneck.0"), ((1, 32, 32), "bottleneck.3"),
                                        ((3, 48, 80), "dec4.3"), ((5, 32, 48), "enc4.0")])
def test_bn_bounds_hold_an_fp32_evaluation_at_small_and_odd_counts(dims, stage, dt):
    """The condition that keeps tests/test_gpu_dataflow.py honest off the production shape: at 45 (3 x 3 x 5), 120 (2 x 6 x
    10) and 4 (1 x 2 x 2) samples per channel, and at 180 and 120 on the levels above, the BatchNorm-family values of a stage
    -- statistics, running statistics, dy, dgamma, dbeta and the conv bias gradient (through which the k-coefficients
    k1 S / M act) -- evaluated in plain fp32 from the same stored inputs, in another summation order, lie within the
    reference's bounds, EVERY element (no masking, no sampling).  The inputs are what a trained-from-init network sees: y
    of unit scale with a per-channel offset, gradients of mixed sign.  With four samples a channel's variance is a chi-square
    of 3 degrees of freedom times the spread of y: never near zero against eps for a continuous y, so no shape had to be
    replaced."""
    from models.model_2 import UNetDC
    g = R.Graph(UNetDC(1, 1))
    st = g.by_name[stage]
    N, H, W = dims
    h, w = H >> st.level, W >> st.level
    P, c = N * h * w, st.cout
    gen = torch.Generator().manual_seed(7 + P)
    y = R.store((torch.randn(P, c, generator=gen, dtype=F64) * (0.5 + torch.rand(c, generator=gen, dtype=F64))
                 + torch.randn(c, generator=gen, dtype=F64)), dt)
    gin = R.store(torch.randn(P, c, generator=gen, dtype=F64) * 1e-3, dt)
    gamma = (torch.rand(c, generator=gen) + 0.5).to(F64)
    beta = (torch.randn(c, generator=gen) * 0.2).to(F64)
    rm, rv = torch.randn(c, generator=gen).to(F64) * 0.1, (torch.rand(c, generator=gen) + 0.5).to(F64)
    S, B = st.name, st.bn_name
    got, y32, g32, colsum, m = _f32_bn_stage(y, gamma, beta, rm, rv, st.eps, st.momentum, gin)
    vals = {f"{S}.y": y, f"P:{B}.weight": gamma, f"P:{B}.bias": beta, f"P:{B}.running_mean": rm, f"P:{B}.running_var": rv}
    get = lambda k: (vals[k], None)                                   # noqa: E731
    fwd = [f"{S}.{k}" for k in ("mean", "rstd", "scale", "shift", "running_mean", "running_var")]
    refs = R.reference(g, fwd, get, dt, "train", dims)
    worst = {}

    def inside(name, value):
        ref, bnd = refs[name]
        bad = X.within_bound(value, ref, bnd, torch.float32 if value.dim() == 1 else dt)
        u = R.unit(dt) if value.dim() > 1 else R.unit(torch.float32)     # as the GPU test reports it: the storage rounding counted in
        worst[name.split(".")[-1]] = float(((value.to(F64).reshape(ref.shape) - ref).abs() / (bnd + u * ref.abs() + 2.0 ** -126)).max())
        assert not bad.any(), f"{name} at {dims}: {int(bad.sum())} of {bad.numel()} fp32-evaluated elements outside the bound"
    for k in fwd:
        inside(k, got[k.split(".", 2)[2]])
    # backward, from the STORED fp32 statistics (teacher forcing), as the kernels read them
    f = torch.float32
    for k in ("mean", "rstd", "scale", "shift"):
        vals[f"{S}.{k}"] = got[k].to(F64)
    vals[f"g:{S}.a"] = gin
    refs = R.reference(g, [f"{S}.dy", f"G:{B}.weight", f"G:{B}.bias", f"G:{st.conv_name}.bias"], get, dt, "train", dims)
    nrm = torch.addcmul(got["shift"], y32, got["scale"])
    gh = torch.where(nrm > 0, g32, torch.zeros_like(g32))
    xh = (y32 - got["mean"]) * got["rstd"]
    s1, s2, s3 = colsum(gh), colsum(gh * xh), colsum(xh)
    k1 = gamma.to(f) * got["rstd"]
    k2, k3 = k1 * s1 / m, k1 * s2 / m
    dy = (k1 * gh - k2) - k3 * xh
    inside(f"{S}.dy", R.store(dy.to(F64), dt).reshape(N, h, w, c))
    inside(f"G:{B}.weight", s2)
    inside(f"G:{B}.bias", s1)
    inside(f"G:{st.conv_name}.bias", -k3 * s3)
    print(f"\n{stage} at {dims} ({P} samples, {dt}): worst fp32-evaluation err / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
