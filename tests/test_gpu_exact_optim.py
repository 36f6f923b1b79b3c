"""fp64-bounded and bit-exact tests of the fused Adam step (csrc/optim.hip adam_pack_kernel through optim.FusedAdam).

The kernel updates p, m and v in place and rewrites both packed weight images of every conv / ConvTranspose2d weight from
the new p; the next forward skips its own re-pack.  So:
  - p, m and v are compared element by element with the fp64 one-step reference from the fp32 state as it was just before
    the step (exact_ref.adam_step), under the per-element bound of exact_ref.adam_bounds, which is derived from the kernel's
    fp32 operation sequence (its docstring).  NaN-strict.  The fixtures span many decades, with exact zeros.
  - both images (w_fwd and w_dgrad) must equal the storage rounding of the host-permuted post-step p, bit for bit.
  - the flat and the torch.cat gradient paths agree bitwise, and the flat gradient buffer is left untouched.
  - a training step that reads the optimizer-written images equals, bitwise, the same step after a forced re-pack.
Parameter sets: UNetDC(3, 1) and UNet(3, 1), so the descriptor table is the production one (all three kinds, plain tensors
with a ragged last 4096-block), in both compute dtypes."""
import pytest
import torch

from tests import exact_ref as X

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.optim import FusedAdam

DEFAULT = (1e-3, (0.9, 0.999), 1e-8)
CUSTOM = (3e-4, (0.8, 0.95), 1e-6)
# (step, hyper-parameters, grad_scale): the first steps (large bias corrections), a late one, the 1/G of a SUM all-reduce
# (1/3 is not a power of two: the scaled gradient rounds), both hyper-parameter sets
CASES = [(1, DEFAULT, 1.0), (2, DEFAULT, 1 / 3), (12345, CUSTOM, 0.5), (1, CUSTOM, 1 / 3), (10000, DEFAULT, 1.0)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(X.INT_VIEW[t.dtype])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_model(arch, dtype, seed=0):
    from models.model import UNet
    from models.model_2 import UNetDC
    torch.manual_seed(seed)
    model = (UNetDC if arch == "unetdc" else UNet)(3, 1).cuda().train()
    model.set_compute_dtype(dtype)
    return model


def batch(seed, n=2, size=64):
    from oracle import recipe
    x = recipe.seeded_input(seed, (n, 3, size, size)).cuda()
    t = recipe.seeded_target(seed + 1, (n, 1, size, size), frac=0.1).cuda()
    return x, t


def train_step(model, opt, x, t):
    """Forward, Focal + Dice loss, backward: (loss, probabilities, every parameter gradient), cloned."""
    from utils.metrics_DC import focal_dice_loss
    opt.zero_grad(set_to_none=True)
    p = model(x)
    loss = focal_dice_loss(p, t, alpha=1.0, gamma=2.0, ratio=0.3)
    loss.backward()
    return loss.detach().clone(), p.detach().clone(), [q.grad.clone() for q in model.parameters()]


def packed_images(model):
    """(parameter, fwd image, dgrad image, kind) of the module's packed weights (engine.PackedWeights.entries)."""
    return [(w, wf, wd, kind) for w, wf, wd, _, _, kind in model._weights.entries()]


def check_images(model, what):
    """Both images of every packed tensor == the storage rounding of the host-permuted p, bit for bit."""
    td = model._weights.tdtype
    names = {id(q): n for n, q in model.named_parameters()}
    for w, wf, wd, kind in packed_images(model):
        ef, ed = X.pack_conv3x3(w.detach()) if kind == 0 else X.pack_convT2x2(w.detach())
        for img, exp, which in ((wf, ef, "w_fwd"), (wd, ed, "w_dgrad")):
            exp = X.to_storage(exp, td).reshape(-1)
            if not same_bits(img, exp):
                bad = (bits(img) != bits(exp)).nonzero().flatten()
                raise AssertionError(f"{what}: {names[id(w)]} {which}: {bad.numel()} of {exp.numel()} elements differ, first at "
                                     f"{int(bad[0])}: {float(img[bad[0]])} != {float(exp[bad[0]])}")


def set_state(model, opt, g, step):
    """A fresh optimizer state: flat gradients (one buffer in parameters() order, as the backward kernels write them), prior
    moments written into the optimizer's flat buffers, the step counter at step - 1.  Returns the flat gradient buffer."""
    params = list(model.parameters())
    if not hasattr(opt, "_m"):
        opt._init_state()
    n = opt._n

    def mag(lo, hi):
        return torch.empty(n, device="cuda").uniform_(lo, hi, generator=g).exp()

    def sign():
        return torch.randint(0, 2, (n,), device="cuda", generator=g).float() * 2 - 1

    flat = sign() * mag(-30.0, 6.0)                           # |g| from 1e-13 to 400
    flat[torch.rand(n, device="cuda", generator=g) < 0.05] = 0.0
    opt._m.copy_(sign() * mag(-25.0, 2.0))
    opt._m[torch.rand(n, device="cuda", generator=g) < 0.05] = 0.0
    opt._v.copy_(mag(-40.0, 4.0))
    opt._v[torch.rand(n, device="cuda", generator=g) < 0.05] = 0.0
    for q, off in zip(params, opt._offs):
        q.grad = flat[off:off + q.numel()].view_as(q)
    opt._step = step - 1
    opt._step_t.fill_(float(step - 1))
    return flat


def flat_params(model):
    return torch.cat([q.detach().reshape(-1) for q in model.parameters()])


def step_and_check(model, opt, step, hyper, gscale, what):
    """One FusedAdam step from the current state; p, m, v within the fp64 bound of the one-step reference, images bit-exact,
    the flat gradient buffer unchanged."""
    lr, (b1, b2), eps = hyper
    group = opt.param_groups[0]
    group["lr"], group["betas"], group["eps"] = lr, (b1, b2), eps
    opt.grad_scale = gscale
    params = list(model.parameters())
    grads = [q.grad for q in params]
    g0 = torch.cat([gr.reshape(-1) for gr in grads])
    p0, m0, v0 = flat_params(model), opt._m.clone(), opt._v.clone()
    graw = [gr.clone() for gr in grads]
    opt.step()
    torch.cuda.synchronize()
    assert all(same_bits(gr, r) for gr, r in zip(grads, graw)), f"{what}: the step wrote into the gradients"
    p1 = flat_params(model)
    names = [n for n, _ in model.named_parameters()]
    offs = opt._offs + [opt._n]
    chunk = 1 << 22
    for i0 in range(0, opt._n, chunk):
        i1 = min(opt._n, i0 + chunk)
        sl = slice(i0, i1)
        ref = X.adam_step(p0[sl], m0[sl], v0[sl], g0[sl], step, lr, b1, b2, eps, gscale)
        bnd = X.adam_bounds(p0[sl], m0[sl], v0[sl], g0[sl], step, lr, b1, b2, eps, gscale)
        for name, got, r, b in (("p", p1[sl], ref[0], bnd[0]), ("m", opt._m[sl], ref[1], bnd[1]), ("v", opt._v[sl], ref[2], bnd[2])):
            bad = X.within_bound(got, r, b, torch.float32)
            if bool(bad.any()):
                k = int(bad.nonzero()[0]) + i0
                t = max(j for j, o in enumerate(offs[:-1]) if o <= k)
                j = k - i0
                raise AssertionError(
                    f"{what}: {name} of {names[t]}[{k - offs[t]}] (of {int(bad.sum())} bad elements) is {float(got[j])!r}, "
                    f"fp64 reference {float(r[j])!r} +- {float(b[j]):.3g}; before the step p={float(p0[k])!r} m={float(m0[k])!r} "
                    f"v={float(v0[k])!r} g={float(g0[k])!r}")
    check_images(model, what)


def restore_params(model, opt, flat):
    with torch.no_grad():
        for q, off in zip(model.parameters(), opt._offs):
            q.copy_(flat[off:off + q.numel()].view_as(q))


def prime(model, seed=3):
    """One eval forward: the module builds its packed weight images (engine.PackedWeights), which the optimizer then owns."""
    x, _ = batch(seed, 1, 32)
    model.eval()
    with torch.no_grad():
        model(x)
    model.train()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["unetdc", "unet"])
def test_fused_adam_step_is_fp64_bounded_and_images_bit_exact(arch, dtype):
    """Every case of CASES from a fresh state: p, m, v within the bound of the fp64 one-step reference, both images bit-exact
    to the new p.  The descriptor table covers all three kinds; the plain tensors end in a ragged 4096-block."""
    model = make_model(arch, dtype)
    prime(model)
    opt = FusedAdam(model)
    kinds = {kind for *_, kind in packed_images(model)}
    assert kinds == {0, 1}, kinds
    packed = {id(w) for w, *_ in packed_images(model)}
    plain = [q for q in model.parameters() if id(q) not in packed]
    assert plain and all(q.numel() % 4096 for q in plain)                # each ends in a ragged 4096-block
    g = torch.Generator(device="cuda").manual_seed(11)
    p_init = flat_params(model)
    for step, hyper, gscale in CASES:
        set_state(model, opt, g, step)
        restore_params(model, opt, p_init)             # every case starts from the initial parameters
        step_and_check(model, opt, step, hyper, gscale, f"{arch}/{dtype} step {step} {hyper} grad_scale {gscale}")
    assert opt._step == CASES[-1][0]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["unetdc", "unet"])
def test_fused_adam_cat_fallback_equals_the_flat_path(arch, dtype):
    """One gradient replaced by a separate tensor (the torch.cat path): bitwise the same p, m, v and images as the flat one."""
    model = make_model(arch, dtype)
    prime(model)
    opt = FusedAdam(model, lr=CUSTOM[0], betas=CUSTOM[1], eps=CUSTOM[2], grad_scale=1 / 3)
    g = torch.Generator(device="cuda").manual_seed(12)
    params = list(model.parameters())
    flat = set_state(model, opt, g, 3)
    p0, m0, v0 = flat_params(model), opt._m.clone(), opt._v.clone()
    opt.step()
    got_flat = (flat_params(model), opt._m.clone(), opt._v.clone(),
                [(wf.clone(), wd.clone()) for _, wf, wd, _ in packed_images(model)])
    restore_params(model, opt, p0)
    opt._m.copy_(m0)
    opt._v.copy_(v0)
    opt._step = 2
    opt._step_t.fill_(2.0)
    packed = {id(w) for w, *_ in packed_images(model)}
    k = next(i for i, q in enumerate(params) if i >= len(params) // 2 and id(q) in packed)    # a packed weight mid-table
    params[k].grad = params[k].grad.clone()
    assert params[k].grad.data_ptr() != flat.data_ptr() + 4 * opt._offs[k]
    opt.step()
    assert same_bits(flat_params(model), got_flat[0]), "p differs between the flat and the torch.cat gradient paths"
    assert same_bits(opt._m, got_flat[1]) and same_bits(opt._v, got_flat[2]), "m / v differ between the two paths"
    for (_, wf, wd, _), (ef, ed) in zip(packed_images(model), got_flat[3]):
        assert same_bits(wf, ef) and same_bits(wd, ed), "packed images differ between the two paths"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_skipped_repack_is_bitwise_a_forced_repack(dtype):
    """After FusedAdam.step() the next forward reads the optimizer-written images (no unetdc_pack_many); the same step after
    a forced re-pack (version counters bumped) reads pack_many's images.  Loss, probabilities and every parameter gradient
    -- the input-gradient convolutions read w_dgrad -- must be bitwise identical."""
    model = make_model("unetdc", dtype)
    opt = FusedAdam(model)
    x, t = batch(21)
    train_step(model, opt, x, t)
    opt.step()
    _lib.start_timing(["unetdc_pack_many", "unetdc_adam_step"])
    try:
        skipped = train_step(model, opt, x, t)
    finally:
        recs_a = _lib.stop_timing()
    for q in model.parameters():
        torch.autograd.graph.increment_version(q)
    _lib.start_timing(["unetdc_pack_many", "unetdc_adam_step"])
    try:
        repacked = train_step(model, opt, x, t)
    finally:
        recs_b = _lib.stop_timing()
    syms_a = [r[0].split("|")[0] for r in recs_a]
    syms_b = [r[0].split("|")[0] for r in recs_b]
    assert "unetdc_pack_many" not in syms_a, f"the step after FusedAdam.step() re-packed: {syms_a}"
    assert "unetdc_pack_many" in syms_b, f"a forced re-pack did not run: {syms_b}"
    assert same_bits(skipped[0], repacked[0]), (float(skipped[0]), float(repacked[0]))
    assert same_bits(skipped[1], repacked[1]), "probabilities differ: the optimizer's w_fwd images are not pack_many's"
    names = [n for n, _ in model.named_parameters()]
    bad = [n for n, a, b in zip(names, skipped[2], repacked[2]) if not same_bits(a, b)]
    assert not bad, f"gradients differ (w_dgrad images not pack_many's): {bad}"


def test_compute_dtype_switch_rebuilds_the_table():
    """bf16 steps, then set_compute_dtype('f32'): a new PackedWeights (new serial) in f32; the next step must write the f32
    images (bit-exact to p) through a rebuilt descriptor table, within the fp64 bound."""
    model = make_model("unetdc", "bf16")
    opt = FusedAdam(model)
    x, t = batch(31)
    for _ in range(2):
        train_step(model, opt, x, t)
        opt.step()
    check_images(model, "bf16 after 2 steps")
    serial = model._weights.serial
    model.set_compute_dtype("f32")
    train_step(model, opt, x, t)
    w = model._weights
    assert w.serial != serial and w.tdtype == torch.float32 and w.dt == _lib.F32
    step_and_check(model, opt, 3, DEFAULT, 1.0, "f32 step after a bf16 -> f32 switch")
    assert opt._table_key[0] == w.serial


def test_adam_abi_rejects_bad_arguments():
    """unetdc_adam_step returns non-zero for step 0, beta1 = 1, lr < 0 and a bad dtype, and leaves p, m, v untouched."""
    model = make_model("unetdc", "bf16")
    prime(model)
    opt = FusedAdam(model)
    g = torch.Generator(device="cuda").manual_seed(41)
    flat = set_state(model, opt, g, 1)
    opt.step()                                        # builds the descriptor table
    torch.cuda.synchronize()
    p0, m0, v0 = flat_params(model), opt._m.clone(), opt._v.clone()
    lib = _lib.load()
    good = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=2, gs=1.0, dtype=_lib.BF16)
    for what, bad in (("step 0", dict(step=0)), ("beta1 = 1", dict(b1=1.0)), ("lr < 0", dict(lr=-1e-3)),
                      ("bad dtype", dict(dtype=2))):
        a = dict(good, **bad)
        rc = lib.unetdc_adam_step(opt._table.data_ptr(), len(list(model.parameters())), opt._blocks, flat.data_ptr(), a["lr"],
                                  a["b1"], a["b2"], a["eps"], a["step"], a["gs"], a["dtype"], stream())
        torch.cuda.synchronize()
        assert rc != 0, f"{what}: accepted"
        assert same_bits(flat_params(model), p0) and same_bits(opt._m, m0) and same_bits(opt._v, v0), f"{what}: state written"
        assert lib.unetdc_last_error().decode(), what
