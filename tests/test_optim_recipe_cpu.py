"""CPU side of the optimizer recipe: the ABI of the three new entry points and their refusals before any
HIP call, FusedAdam's PyTorch formulas with decay / clipping / guard / EMA against torch.optim.AdamW + clip_grad_norm_, the
learning-rate schedules against their closed forms and torch's ReduceLROnPlateau, and the flags of the training entry point."""
import ctypes
import math
import os

import pytest
import torch

from tests import exact_ref as X
from tests import optim_recipe_ref as R

NEW = ("unetdc_grad_norm_workspace", "unetdc_grad_norm", "unetdc_adam_step_ex")


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_header_and_ctypes_table_agree_on_the_new_symbols(lib):
    from unet_dc_segmentation_amd import _lib, optim
    hdr = X.parse_header()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(hdr[name]) == len(_lib.SIGNATURES[name][1]), (name, hdr[name])
    assert hdr["unetdc_adam_step_ex"][:11] == hdr["unetdc_adam_step"][:11]           # the plain step's arguments, then the recipe's
    assert hdr["unetdc_adam_step_ex"][11:] == ("ctl_dev", "weight_decay", "ema_base", "m_base", "ema_decay", "s")
    assert optim._DESC == R.DESC and optim._CTL == R.CTL and optim._DESC.names[-1] == "flags"
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unetdc_hip.h")).read()
    assert "int32_t flags;" in src and "} unetdc_step_ctl;" in src


def test_grad_norm_workspace_query(lib):
    q = lib.unetdc_grad_norm_workspace
    assert q(0) == 0 and q(-5) == 0
    assert q(1) == 8 and q(R.NORM_BLOCK) == 8 and q(R.NORM_BLOCK + 1) == 16
    assert q(R.NORM_PARTS * R.NORM_BLOCK) == 8 * R.NORM_PARTS == q(R.NORM_PARTS * R.NORM_BLOCK + 1) == q(1 << 40)


def test_refusals_come_before_any_hip_call(lib):
    """Host memory stands in for device memory: every call here must return before the first launch."""
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    g, ctl, ws = a, a + 4096, a + 8192
    n = 10000
    need = lib.unetdc_grad_norm_workspace(n)
    assert need == 24
    rc = lib.unetdc_grad_norm(g + 4, n, 1.0, 1.0, ctl, ws, need, None)
    assert rc == -1 and b"16-byte aligned" in lib.unetdc_last_error(), (rc, lib.unetdc_last_error())
    for bad_n in (0, -3):
        rc = lib.unetdc_grad_norm(g, bad_n, 1.0, 1.0, ctl, ws, need, None)
        assert rc == -1 and b"grad_norm: n" in lib.unetdc_last_error(), (rc, lib.unetdc_last_error())
    rc = lib.unetdc_grad_norm(g, n, 1.0, 1.0, ctl, ws, need - 1, None)
    err = lib.unetdc_last_error()
    assert rc == -3 and err.startswith(b"grad_norm") and b"workspace too small" in err, (rc, err)
    rc = lib.unetdc_grad_norm(g, n, float("inf"), 1.0, ctl, ws, need, None)
    assert rc == -1 and b"finite" in lib.unetdc_last_error()
    rc = lib.unetdc_grad_norm(None, n, 1.0, 1.0, ctl, ws, need, None)
    assert rc == -1 and b"null" in lib.unetdc_last_error()
    # the extended step: what the plain step refuses, and the recipe's own arguments
    ok = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, gs=1.0, dtype=0, ctl=None, wd=0.0, ema=None, mb=None, d=0.0)
    for what, bad, msg in (("step 0", dict(step=0), b"hyper"), ("dtype", dict(dtype=2), b"dtype"),
                           ("negative decay", dict(wd=-1.0), b"weight_decay"), ("lr * wd >= 1", dict(wd=1000.0), b"weight_decay"),
                           ("ema without m_base", dict(ema=a), b"EMA"), ("ema decay 2", dict(ema=a, mb=a, d=2.0), b"EMA"),
                           ("misaligned ctl", dict(ctl=ctl + 4), b"8-byte")):
        k = dict(ok, **bad)
        rc = lib.unetdc_adam_step_ex(a, 1, 1, g, k["lr"], k["b1"], k["b2"], k["eps"], k["step"], k["gs"], k["dtype"], k["ctl"],
                                     k["wd"], k["ema"], k["mb"], k["d"], None)
        assert rc == -1 and msg in lib.unetdc_last_error(), (what, rc, lib.unetdc_last_error())


# ---------------------------------------------------------------------------------------------------- FusedAdam on CPU tensors
def twins(seed=0):
    from models.model_2 import UNetDC
    torch.manual_seed(seed)
    a, b = UNetDC(1, 1), UNetDC(1, 1)
    b.load_state_dict(a.state_dict())
    return a, b


def set_grads(g, scale, *models):
    for ps in zip(*(m.parameters() for m in models)):
        gr = torch.randn(ps[0].shape, generator=g) * scale
        for p in ps:
            p.grad = gr.clone()


def close(a, b):
    return all(torch.allclose(pa, pb, rtol=1e-6, atol=1e-8) for pa, pb in zip(a.parameters(), b.parameters()))


def test_fused_adam_cpu_recipe_matches_adamw_and_clip_grad_norm():
    """weight_decay on all parameters + clip_norm against torch.optim.AdamW + clip_grad_norm_, 3 steps on UNetDC(1, 1), under
    the criterion of the plain-Adam CPU test; then the state into torch.optim.AdamW and back."""
    from unet_dc_segmentation_amd.optim import FusedAdam
    a, b = twins()
    oa = FusedAdam(a, lr=1e-2, weight_decay=0.05, decay="all", clip_norm=1.0)
    ob = torch.optim.AdamW(b.parameters(), lr=1e-2, weight_decay=0.05)
    g = torch.Generator().manual_seed(1)
    for scale in (1.0, 1e-4, 3.0):                        # steps 1 and 3 clip (the norm of ~7.8e6 unit normals), step 2 does not
        set_grads(g, scale, a, b)
        raw = [p.grad.clone() for p in a.parameters()]
        oa.step()
        assert all(torch.equal(p.grad, r) for p, r in zip(a.parameters(), raw)), "the step wrote into the gradients"
        torch.nn.utils.clip_grad_norm_(b.parameters(), 1.0)
        ob.step()
        assert close(a, b)
    s = oa.recipe_stats()
    assert (s["steps"], s["clipped"], s["skipped"]) == (3, 2, 0) and s["grad_norm_mean"] > 1.0
    sda, sdb = oa.state_dict(), ob.state_dict()
    ga = sda["param_groups"][0]
    assert ga.keys() == sdb["param_groups"][0].keys() and ga["weight_decay"] == 0.05 and ga["decoupled_weight_decay"] is True
    oc = torch.optim.AdamW(a.parameters(), lr=1e-2, weight_decay=0.05, foreach=False)
    oc.load_state_dict(sda)
    set_grads(g, 1e-4, a, b)                              # below the clip: AdamW alone takes the step FusedAdam would
    oc.step()
    ob.step()
    assert close(a, b)
    od = FusedAdam(a, lr=1e-2, weight_decay=0.05, decay="all", clip_norm=1.0)
    od.load_state_dict(ob.state_dict())
    assert od._step == 4 and od.param_groups[0]["weight_decay"] == 0.05
    set_grads(g, 2.0, a, b)
    od.step()
    torch.nn.utils.clip_grad_norm_(b.parameters(), 1.0)
    ob.step()
    assert close(a, b)
    # a plain torch.optim.Adam state still loads (and switches the decay off, as its group says)
    oe = FusedAdam(a, lr=1e-2, weight_decay=0.05)
    oe.load_state_dict(torch.optim.Adam(a.parameters(), lr=1e-2).state_dict())
    assert oe.param_groups[0]["weight_decay"] == 0
    with pytest.raises(ValueError, match="decoupled"):
        oe.load_state_dict(torch.optim.Adam(a.parameters(), lr=1e-2, weight_decay=0.1).state_dict())


def test_decay_weights_leaves_biases_and_batchnorm_alone():
    """decay='weights' with zero gradients and zero moments: Adam's own update is 0 / (0 + eps) = 0, so exactly the tensors
    with dim() >= 2 shrink by 1 - lr * wd."""
    from unet_dc_segmentation_amd.optim import FusedAdam
    a, b = twins(3)
    o = FusedAdam(a, lr=0.5, weight_decay=0.5)
    for p in a.parameters():
        p.grad = torch.zeros_like(p)
    o.step()
    for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
        want = pb * 0.75 if pb.dim() >= 2 else pb
        assert torch.equal(pa, want), name
    assert any(p.dim() < 2 for p in a.parameters())


def test_cpu_nonfinite_step_is_dropped_and_the_next_proceeds():
    from unet_dc_segmentation_amd.optim import FusedAdam
    a, _ = twins(4)
    o = FusedAdam(a, lr=1e-2, weight_decay=0.01, ema_decay=0.9, skip_nonfinite=True)
    g = torch.Generator().manual_seed(5)
    set_grads(g, 1.0, a)
    o.step()
    snap = lambda: [t.clone() for t in (*a.parameters(), o._m, o._v, o._ema)]      # noqa: E731
    before = snap()
    set_grads(g, 1.0, a)
    list(a.parameters())[7].grad.view(-1)[-1] = float("nan")
    o.step()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(snap(), before))
    assert o.recipe_stats()["skipped"] == 1 and o._step == 2            # the host counter advances on a dropped step too
    set_grads(g, 1.0, a)
    o.step()
    after = snap()
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[-1], before[-1])
    s = o.recipe_stats()
    assert (s["steps"], s["clipped"], s["skipped"]) == (3, 0, 1) and math.isfinite(s["grad_norm_mean"])


def test_ema_follows_its_rule_and_ema_weights_swaps_and_restores():
    from unet_dc_segmentation_amd.optim import FusedAdam, ema_decay_at
    a, b = twins(6)
    o = FusedAdam(a, lr=1e-2, ema_decay=0.999)
    g = torch.Generator().manual_seed(7)
    e = [p.detach().clone().double() for p in b.parameters()]             # the EMA starts as a copy of the parameters
    for t in (1, 2, 3):
        set_grads(g, 1.0, a)
        o.step()
        d = ema_decay_at(0.999, t)
        assert d == min(0.999, (1 + t) / (10 + t)) == R.ema_decay_at(0.999, t)
        e = [x + (1 - d) * (p.detach().double() - x) for x, p in zip(e, a.parameters())]
    assert all(torch.allclose(v.double(), x, rtol=1e-6, atol=1e-8) for v, x in zip(o.ema_tensors(), e))
    saved = [p.detach().clone() for p in a.parameters()]
    versions = [p._version for p in a.parameters()]
    stats = {k: v.clone() for k, v in a.state_dict().items() if "running" in k}
    with o.ema_weights():
        assert all(torch.equal(p, v) for p, v in zip(a.parameters(), o.ema_tensors()))
        assert not all(torch.equal(p, s) for p, s in zip(a.parameters(), saved))
        assert all(p._version > v0 for p, v0 in zip(a.parameters(), versions))      # the engine's re-pack rule sees the swap
    assert all(torch.equal(p.view(torch.int32), s.view(torch.int32)) for p, s in zip(a.parameters(), saved))
    assert all(torch.equal(v, a.state_dict()[k]) for k, v in stats.items())
    # the EMA buffer rides in state_dict() under its own top-level key and comes back
    sd = o.state_dict()
    assert sd["ema"].numel() == sum(p.numel() for p in a.parameters())
    o2 = FusedAdam(a, lr=1e-2, ema_decay=0.999)
    o2.load_state_dict(sd)
    assert torch.equal(o2._ema, o._ema) and o2._ema.data_ptr() != o._ema.data_ptr()
    with pytest.raises(RuntimeError, match="ema_decay"):
        FusedAdam(a).ema_tensors()


# ---------------------------------------------------------------------------------------------------- schedules
def test_cosine_schedule_endpoints_and_warmup_against_the_closed_form():
    from utils.lr_schedule import LRSchedule
    base, lo, T, W = 1e-3, 1e-5, 100, 10
    s = LRSchedule("cosine", base, T, W, lo)
    assert [s.lr_at(k) for k in range(W)] == [base * ((k + 1) / W) for k in range(W)]        # (cos(0) = 1 exactly)
    assert s.lr_at(W) == base and s.lr_at(T) == lo == s.lr_at(T + 50)
    mid = (T + W) // 2
    assert abs(s.lr_at(mid) - (lo + (base - lo) / 2)) < 1e-18
    for k in range(T + 1):
        assert s.lr_at(k) == R.cosine_lr(k, base, lo, T, W), k
    assert all(s.lr_at(k + 1) < s.lr_at(k) for k in range(W, T - 1))
    c = LRSchedule("constant", base, 0, 4)
    assert [c.lr_at(k) for k in range(6)] == [base * 0.25, base * 0.5, base * 0.75, base, base, base]
    with pytest.raises(ValueError):
        LRSchedule("cosine", base, 10, 10)
    with pytest.raises(ValueError):
        LRSchedule("linear", base)


def test_plateau_schedule_is_torch_reduce_lr_on_plateau():
    from utils.lr_schedule import LRSchedule
    losses = [1.0, 0.9, 0.9, 0.91, 0.9, 0.95, 0.9, 0.9, 0.9, 0.89999, 0.5, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6,
              0.6, float("nan"), 0.6, 0.6, 0.6, 0.6, 0.6, 0.4] + [0.45] * 40
    for lr_min in (0.0, 2e-4):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=1e-3)
        ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=5, min_lr=lr_min)
        s = LRSchedule("plateau", 1e-3, 0, 0, lr_min)
        seen = set()
        for v in losses:
            ref.step(v)
            s.epoch_end(v)
            assert s.lr_at(0) == opt.param_groups[0]["lr"], (v, s.lr_at(0), opt.param_groups[0]["lr"])
            seen.add(s.lr_at(0))
        assert len(seen) >= 3 and min(seen) >= lr_min


# ---------------------------------------------------------------------------------------------------- entry point
RUN = ["--synthetic", "--synthetic_len", "10", "--img_size", "32", "--batch", "2", "--epochs", "2", "--workers", "0",
       "--in_channels", "1", "--device", "cpu", "--no_test_eval"]
PARENT_KEYS = {"epoch", "train_loss", "val_loss", "train_dice", "val_dice", "train_acc", "val_acc", "images_per_sec"}


def test_entry_point_with_every_recipe_flag(tmp_path):
    import train_DC_focal as t
    hist = t.main(RUN + ["--ckpt_path", str(tmp_path / "a.pth"), "--weight_decay", "0.01", "--decay_all", "--clip_grad", "0.5",
                         "--ema", "0.99", "--lr_schedule", "cosine", "--warmup_steps", "2", "--lr_min", "1e-5"])
    assert len(hist) == 2
    for rec in hist:
        assert set(rec) == PARENT_KEYS | {"lr", "grad_norm_mean", "clipped_steps", "skipped_steps"}
        assert all(math.isfinite(float(v)) for v in rec.values()), rec
        assert rec["skipped_steps"] == 0 and 0 <= rec["clipped_steps"] <= 3 and rec["grad_norm_mean"] > 0
    # 6 training tiles at batch 2: 3 steps an epoch, 6 planned; the record holds the rate of the epoch's last step
    assert hist[0]["lr"] == R.cosine_lr(2, 1e-3, 1e-5, 6, 2) and hist[1]["lr"] == R.cosine_lr(5, 1e-3, 1e-5, 6, 2)
    hist = t.main(RUN + ["--ckpt_path", str(tmp_path / "b.pth"), "--lr_schedule", "plateau"])
    assert [set(rec) for rec in hist] == [PARENT_KEYS | {"lr"}] * 2 and hist[0]["lr"] == 1e-3


def test_entry_point_without_flags_is_the_plain_adam_run(tmp_path, monkeypatch):
    """No new key, and the values of a parent-style run: the reference's torch.optim.Adam(lr) on the CPU, constructed exactly
    once and never handed another learning rate."""
    import train_DC_focal as t
    made = []
    orig = torch.optim.Adam

    class Spy(orig):
        def __init__(self, *a, **k):
            made.append(k)
            super().__init__(*a, **k)

    monkeypatch.setattr(torch.optim, "Adam", Spy)
    h1 = t.main(RUN + ["--ckpt_path", str(tmp_path / "a.pth")])
    assert len(made) == 1 and made[0]["lr"] == 1e-3
    h2 = t.main(RUN + ["--ckpt_path", str(tmp_path / "b.pth"), "--weight_decay", "0", "--lr_schedule", "constant",
                       "--warmup_steps", "0"])
    assert len(made) == 2
    strip = lambda h: [{k: v for k, v in rec.items() if k != "images_per_sec"} for rec in h]     # noqa: E731
    assert [set(rec) for rec in h1] == [PARENT_KEYS] * 2
    assert strip(h1) == strip(h2)


def test_entry_point_refuses_recipe_flags_with_the_torch_optimizer():
    import train_DC_focal as t
    with pytest.raises(SystemExit, match="--clip_grad.*cannot run with --optimizer torch"):
        t.main(["--synthetic", "--device", "cpu", "--optimizer", "torch", "--clip_grad", "1"])
    for bad in (["--decay_all"], ["--clip_grad", "0"], ["--ema", "1.0"], ["--lr_min", "1e-4"], ["--warmup_steps", "-1"]):
        with pytest.raises(SystemExit):
            t.main(["--synthetic", "--device", "cpu"] + bad)
