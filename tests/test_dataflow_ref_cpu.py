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


@pytest.mark.parametrize("arch,shape", [("unetdc", (2, 1, 32, 32)), ("unetdc", (1, 3, 64, 64)), ("unet", (2, 1, 32, 32)),
                                        ("unet", (1, 3, 64, 64))])
def test_fp64_chain_reproduces_the_module(arch, shape):
    from models.model import UNet
    from models.model_2 import UNetDC
    from utils.metrics_DC import focal_dice_loss
    torch.manual_seed(3)
    n, c, h, w = shape
    model = (UNetDC if arch == "unetdc" else UNet)(c, 1).double().train()
    gen = torch.Generator().manual_seed(4)
    x = torch.rand(shape, generator=gen, dtype=F64)
    t = (torch.rand(n, 1, h, w, generator=gen) < 0.3).to(F64)
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
