"""GPU: the separation weight map and the border-weighted loss (csrc/border.hip, loss.hip) through the C
ABI.  Every output of unetdc_border_weights sits between canaries, its workspace is pre-filled with garbage, and the integer
planes are compared bit for bit with the brute-force window search of tests/border_ref.py."""
import functools

import numpy as np
import pytest
import torch

from tests import border_ref as ref
from tests import workspace_states as wss
from tests.image_canaries import Canaried, canaried_like, check_all

pytestmark = pytest.mark.gpu

RADII = (1, 3, 20, 64)
NOISE = [(h, w, dens, 100 + 10 * k + j) for k, (h, w) in enumerate(((70, 131), (96, 128))) for j, dens in enumerate((0.02, 0.1, 0.3))]
W0, SIGMA = 10.0, 5.0


@functools.lru_cache(maxsize=None)
def noise_mask(h, w, dens, seed):
    return ref.noise_mask(h, w, dens, seed)


@functools.lru_cache(maxsize=None)
def noise_ref(h, w, dens, seed, R):
    return ref.brute_planes(noise_mask(h, w, dens, seed), R)


def stream():
    return torch.cuda.current_stream().cuda_stream


def run(masks, R, w0=W0, sigma=SIGMA, planes=True, state="a5", stale=None, skew=0):
    """unetdc_border_weights on masks [n, h, w] float32 -> (weights float32, D1, D2 int32 or None, the workspace view).  Outputs
    and workspace are Canaried views; the workspace holds `state` before the call."""
    from unet_dc_segmentation_amd import _lib
    masks = np.ascontiguousarray(masks, np.float32)
    n, h, w = masks.shape
    nbytes = _lib.load().unetdc_border_weights_workspace(n, h, w, R)
    assert nbytes == n * h * w * 14 + 64
    t = canaried_like(masks, skew=skew)
    ow = Canaried(masks.size * 4, skew=skew)
    o1 = Canaried(masks.size * 4 if planes else 0, skew=skew)
    o2 = Canaried(masks.size * 4 if planes else 0, skew=skew)
    ws = wss.prepare(Canaried(nbytes), state, stale)
    _lib.call("unetdc_border_weights", t.ptr, n, h, w, w0, sigma, R, ow.ptr, o1.ptr if planes else None, o2.ptr if planes else None,
              ws.ptr, nbytes, stream())
    torch.cuda.synchronize()
    check_all(t, ow, o1, o2, ws)
    assert np.array_equal(t.numpy(np.float32, n, h, w), masks)                     # the input is read only
    return (ow.numpy(np.float32, n, h, w), o1.numpy(np.int32, n, h, w) if planes else None,
            o2.numpy(np.int32, n, h, w) if planes else None, ws)


def check_weights(wt, d1, d2, R, w0=W0, sigma=SIGMA):
    """The float weight against the fp64 formula on the device's own integer planes: exactly 1.0f outside the term; inside, the
    border term within term_bound (relative) plus the rounding of the final sum 1 + term to fp32 (half an ulp: 2^-24 w).
    -> the largest error seen, in units of that allowance, and relative to the term."""
    on, term = ref.weight64(d1, d2, w0, sigma, R)
    assert np.all(wt[~on] == np.float32(1.0))
    if not on.any():
        return 0.0, 0.0
    w64 = 1.0 + term[on]
    err = np.abs(wt[on].astype(np.float64) - w64)
    allowed = ref.term_bound(R, sigma) * term[on] + 2.0 ** -24 * w64
    assert np.all(err <= allowed), (float((err / allowed).max()), R)
    big = term[on] > 0.05 * w0                                                     # where the final rounding is small next to the term
    return float((err / allowed).max()), float((err[big] / term[on][big]).max()) if big.any() else 0.0


@pytest.mark.parametrize("R", RADII)
def test_edge_cases_bit_exact(R):
    stale = None
    for k, (name, m) in enumerate(ref.edge_cases(R)):
        state = wss.STATES[k % len(wss.STATES)] if stale is not None else "a5"
        wt, d1, d2, ws = run(m[None], R, state=state, stale=stale, skew=(16 * k) % 256)
        stale = ws.u8.clone()                                                      # what the next geometry finds in its workspace
        b1, b2 = ref.brute_planes(m, R)
        assert np.array_equal(d1[0], b1) and np.array_equal(d2[0], b2), (name, R, state)
        check_weights(wt, d1, d2, R)
        if name.startswith(("empty", "full", "one_")):
            assert np.all(wt == np.float32(1.0)) and np.all(d2[0][m < 0.5] == ref.INF), name
        if name == "second_at_R" and R > 1:
            on, term = ref.weight64(d1, d2, W0, SIGMA, R)                          # the cut-off is inclusive: the pixel carries a
            assert d2[0, 2, 1] == R * R and on[0, 2, 1]                            # term (which fp32 can show next to 1 up to R = 20)
            assert wt[0, 2, 1] > 1.0 or term[0, 2, 1] < 2.0 ** -23
        if name == "second_past_R" and R > 1:
            assert d2[0, 2, 1] == R * R + 1 and wt[0, 2, 1] == 1.0
        if name == "behind_in_column" and R >= 4:
            assert (d1[0, 5, 2], d2[0, 5, 2]) == (4, 16)                           # one candidate per column would lose B


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("case", NOISE, ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}")
def test_noise_masks_bit_exact(case, R):
    m = noise_mask(*case)
    wt, d1, d2, _ = run(m[None], R, state="ones")
    b1, b2 = noise_ref(*case, R)
    assert np.array_equal(d1[0], b1) and np.array_equal(d2[0], b2)
    units, rel = check_weights(wt, d1, d2, R)
    print(f"\n border term, R {R}, {case[0]}x{case[1]} density {case[2]}: largest error {units:.3f} of the allowance, "
          f"{rel:.3e} relative to the term (bound {ref.term_bound(R, SIGMA):.3e})")
    # without the planes: the same weights
    w2, _, _, _ = run(m[None], R, planes=False, state="zero")
    assert np.array_equal(w2.view(np.uint32), wt.view(np.uint32))


def test_other_sigma_and_w0():
    m = noise_mask(*NOISE[1])
    for w0, sigma, R in ((0.0, 5.0, 20), (3.5, 1.0, 4), (10.0, 16.0, 64), (10.0, 0.25, 1)):
        wt, d1, d2, _ = run(m[None], R, w0=w0, sigma=sigma)
        check_weights(wt, d1, d2, R, w0, sigma)
        if w0 == 0.0:
            assert np.all(wt == np.float32(1.0))


def test_three_images_do_not_leak_and_two_calls_are_bit_equal():
    h, w, R = 70, 131, 20
    assert NOISE[2][:3] == (h, w, 0.3)
    dense = noise_mask(*NOISE[2])
    batch = np.stack([dense, np.zeros((h, w), np.float32), np.ones((h, w), np.float32)])
    wt, d1, d2, ws = run(batch, R, state="a5")
    b1, b2 = noise_ref(*NOISE[2], R)
    assert np.array_equal(d1[0], b1) and np.array_equal(d2[0], b2)
    assert np.all(d1[1] == ref.INF) and np.all(d2[1] == ref.INF) and np.all(d1[2] == 0) and np.all(d2[2] == 0)
    assert np.all(wt[1:] == np.float32(1.0))
    # the other order (the dense image last, next to the full one), another workspace state: the same planes per image
    w2, e1, e2, _ = run(batch[::-1], R, state="stale", stale=ws.u8.clone())
    assert np.array_equal(e1[::-1], d1) and np.array_equal(e2[::-1], d2) and np.array_equal(w2[::-1].view(np.uint32), wt.view(np.uint32))
    w3, f1, f2, _ = run(batch, R, state="ones")
    assert np.array_equal(f1, d1) and np.array_equal(f2, d2) and np.array_equal(w3.view(np.uint32), wt.view(np.uint32))


def test_python_wrapper_matches_the_host_path():
    from unet_dc_segmentation_amd.border import border_weights, workspace_bytes
    from utils.border_weights import border_weights_numpy
    m = np.stack([noise_mask(*NOISE[0]), noise_mask(*NOISE[1])])[:, None]          # [2, 1, 70, 131]
    t = torch.from_numpy(m).cuda()
    wt, d1, d2 = border_weights(t, 10.0, planes=True)
    nw, n1, n2 = border_weights_numpy(m, 10.0, planes=True)
    assert wt.shape == t.shape and np.array_equal(d1.cpu().numpy(), n1) and np.array_equal(d2.cpu().numpy(), n2)
    np.testing.assert_allclose(wt.cpu().numpy(), nw, rtol=ref.term_bound(20, 5.0) + 2.0 ** -23, atol=0)
    out = torch.empty_like(wt)
    ws = torch.empty(workspace_bytes(2, 70, 131, 20), dtype=torch.uint8, device="cuda")
    assert border_weights(t.bool(), 10.0, out=out, workspace=ws) is out and torch.equal(out, wt)
    assert not wt.requires_grad


# ---- the weighted loss -------------------------------------------------------------------------------------------------------

def loss_abi(p, t, wt, alpha, gamma, ratio, gout=3.0):
    """(loss, coef, dp) of the C ABI calls on fp32 CUDA tensors [N, C, H, W]; wt None: the unweighted entry points."""
    from unet_dc_segmentation_amd import _lib
    nimg, hw = p.shape[0] * p.shape[1], p.shape[2] * p.shape[3]
    nbytes = _lib.load().unetdc_focal_dice_loss_workspace(nimg, hw)
    ws = torch.full((max(int(nbytes), 16),), 0xA5, dtype=torch.uint8, device="cuda")
    loss = torch.full((), float("nan"), device="cuda")
    coef = torch.full((nimg * 2,), float("nan"), device="cuda")
    dp = torch.full_like(p, float("nan"))
    g = torch.tensor(gout, device="cuda")
    if wt is None:
        _lib.call("unetdc_focal_dice_loss_fwd", p.data_ptr(), t.data_ptr(), loss.data_ptr(), coef.data_ptr(), ws.data_ptr(), nbytes,
                  nimg, hw, alpha, gamma, ratio, 1e-7, stream())
        _lib.call("unetdc_focal_dice_loss_bwd", p.data_ptr(), t.data_ptr(), coef.data_ptr(), g.data_ptr(), dp.data_ptr(), nimg, hw,
                  alpha, gamma, ratio, stream())
    else:
        _lib.call("unetdc_focal_dice_loss_w_fwd", p.data_ptr(), t.data_ptr(), wt.data_ptr(), loss.data_ptr(), coef.data_ptr(),
                  ws.data_ptr(), nbytes, nimg, hw, alpha, gamma, ratio, 1e-7, stream())
        _lib.call("unetdc_focal_dice_loss_w_bwd", p.data_ptr(), t.data_ptr(), wt.data_ptr(), coef.data_ptr(), g.data_ptr(),
                  dp.data_ptr(), nimg, hw, alpha, gamma, ratio, stream())
    torch.cuda.synchronize()
    return loss.cpu(), coef.cpu(), dp.cpu()


def loss_case(shape, seed=23):
    """The random case of tests/test_gpu_ops.py::test_fused_focal_dice_loss (its log-clamp probabilities included) at `shape`."""
    g = torch.Generator().manual_seed(seed)
    pr = torch.rand(*shape, generator=g)
    clamps = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7])
    k = min(4, shape[-1])
    pr[0, 0, 0, :k] = clamps[:k]
    tg = (torch.rand(*shape, generator=g) < 0.3).float()
    return pr, tg


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("shape", [(3, 2, 40, 56), (3, 2, 1, 1), (3, 2, 1, 2049)], ids=["40x56", "hw1", "hw2049"])
def test_weight_of_ones_is_the_unweighted_loss_bit_for_bit(shape, gamma):
    pr, tg = loss_case(shape)
    p, t = pr.cuda(), tg.cuda()
    l0, c0, d0 = loss_abi(p, t, None, 0.75, gamma, 0.4)
    l1, c1, d1 = loss_abi(p, t, torch.ones_like(p), 0.75, gamma, 0.4)
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(c0), bits(c1)) and torch.equal(bits(d0), bits(d1))
    assert torch.isfinite(l0) and torch.isfinite(c0).all()


def two_droplet_target(shape):
    t = torch.zeros(shape)
    t[..., 10:20, 8:18] = 1
    t[..., 12:25, 21:30] = 1                                                       # a 3-pixel gap between the two
    return t


@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("kind", ["border_map", "random"])
def test_weighted_loss_matches_the_pytorch_formulation(kind, gamma):
    from unet_dc_segmentation_amd.border import border_weights
    from utils import metrics_DC as M
    pr, tg = loss_case((3, 2, 40, 56))
    if kind == "border_map":
        # (the map of a two-droplet mask on that case's own random targets: its clamped probabilities keep the targets they have
        # in tests/test_gpu_ops.py, where the fused kernel and PyTorch agree on which gradients are finite)
        wt = border_weights(two_droplet_target((3, 2, 40, 56)).cuda(), 10.0)
        assert float(wt.max()) > 5.0 and float(wt.min()) == 1.0
    else:
        wt = (1.0 + 10.0 * torch.rand(3, 2, 40, 56, generator=torch.Generator().manual_seed(29))).cuda()
    a = pr.clone().cuda().requires_grad_(True)
    b = pr.clone().cuda().requires_grad_(True)
    lf = M.focal_dice_loss(a, tg.cuda(), alpha=0.75, gamma=gamma, ratio=0.4, weight=wt)
    assert type(lf.grad_fn).__name__.startswith("_FocalDiceWeighted")              # the HIP path, not the fall-back
    focal = M.FocalLoss(alpha=0.75, gamma=gamma, reduction="none")(b, tg.cuda())
    lt = 0.4 * (wt * focal).mean() + 0.6 * M.dice_loss(b, tg.cuda())
    print(f"\n weighted loss ({kind}, gamma {gamma}): HIP {lf.item():.8f}, PyTorch {lt.item():.8f}")
    assert abs(lf.item() - lt.item()) < 2e-6 * max(1.0, abs(lt.item()))
    (lf * 3.0).backward()
    (lt * 3.0).backward()
    fin = torch.isfinite(b.grad)
    assert torch.equal(torch.isfinite(a.grad), fin)
    assert float((a.grad[fin] - b.grad[fin]).abs().max()) < 1e-6 * float(b.grad[fin].abs().max()) + 1e-9


def test_one_training_step_with_border_weights():
    """model -> weighted loss -> backward at 2 x 1 x 64 x 64 in fp32: every parameter gradient against the same step with the
    weighted PyTorch loss.  Band: 2e-4 of the largest gradient of the tensor, the relative band of tests/test_gpu_training.py
    for the first fp32 steps (same arithmetic up to the evaluation order of the loss)."""
    from models.model_2 import UNetDC
    from unet_dc_segmentation_amd.border import border_weights
    from utils import metrics_DC as M
    torch.manual_seed(3)
    model = UNetDC(1, 1).cuda().train()
    model.set_compute_dtype("f32")
    x = torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(4)).cuda()
    t = two_droplet_target((2, 1, 64, 64)).cuda()
    wt = border_weights(t, 10)
    assert float(wt.max()) > 5.0
    grads = []
    for hip in (True, False):
        model.zero_grad(set_to_none=True)
        p = model(x)
        if hip:
            loss = M.focal_dice_loss(p, t, weight=wt)
            assert type(loss.grad_fn).__name__.startswith("_FocalDiceWeighted")
        else:
            loss = 0.3 * (wt * M.FocalLoss(alpha=1.0, gamma=2.0, reduction="none")(p, t)).mean() + 0.7 * M.dice_loss(p, t)
        loss.backward()
        grads.append((float(loss.item()), {k: v.grad.detach().clone() for k, v in model.named_parameters()}))
    (la, ga), (lb, gb) = grads
    assert abs(la - lb) < 2e-6 * max(1.0, abs(lb))
    worst = 0.0
    for k in gb:
        scale = float(gb[k].abs().max())
        gap = float((ga[k] - gb[k]).abs().max())
        worst = max(worst, gap / max(scale, 1e-30))
        assert torch.isfinite(ga[k]).all() and gap <= 2e-4 * scale + 1e-12, (k, gap, scale)
    print(f"\n one step with border weights: loss {la:.7f} / {lb:.7f}, largest gradient gap {worst:.2e} of the tensor's maximum")
    plain = M.focal_dice_loss(model(x), t)
    assert abs(float(plain.item()) - la) > 1e-4                                    # the weights do change the loss


def write_pairs(d, n=5, size=64):
    """n synthetic droplet tiles as PNG pairs (what --device_data caches): -> (image dir, mask dir)."""
    from PIL import Image
    from utils.data_loader import SyntheticDropletDataset
    ds = SyntheticDropletDataset(n, size, 3, seed=42)
    ind, md = d / "images", d / "masks"
    ind.mkdir()
    md.mkdir()
    for i in range(n):
        img, mask = ds[i][0].numpy(), ds[i][1].numpy()
        Image.fromarray((np.clip(img, 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)).save(ind / f"t_{i}.png")
        Image.fromarray((mask[0] * 255).astype(np.uint8)).save(md / f"t_{i}.png")
    return str(ind), str(md)


@pytest.mark.parametrize("device_data", [False, True], ids=["host_loader", "device_data"])
def test_training_entry_point_with_the_flag(device_data, tmp_path, capsys):
    """train_DC_focal.main for one epoch of 64 x 64 tiles at batch 2, with and without --border_weight: a finite training loss
    that differs from the flag-less run's, the same validation loss definition (unweighted), and the start-up line.  The host
    loader runs on --synthetic tiles; --device_data caches files and refuses --synthetic, so it gets the same kind of tiles as
    PNG pairs."""
    import train_DC_focal as T
    common = ["--batch", "2", "--img_size", "64", "--epochs", "1", "--workers", "0", "--no_test_eval", "--ckpt_path",
              str(tmp_path / "ck.pth")]
    if device_data:
        ind, md = write_pairs(tmp_path)
        common += ["--image_dir", ind, "--mask_dir", md, "--device_data"]
    else:
        common += ["--synthetic", "--synthetic_len", "4"]
    plain = T.main(common)
    assert "--border_weight" not in capsys.readouterr().out
    again = T.main(common)
    weighted = T.main(common + ["--border_weight"])
    assert "--border_weight 10" in capsys.readouterr().out
    assert plain[0]["train_loss"] == again[0]["train_loss"]                        # the flag-less run is reproducible ...
    assert np.isfinite(weighted[0]["train_loss"]) and np.isfinite(weighted[0]["val_loss"])
    assert weighted[0]["train_loss"] > plain[0]["train_loss"]                      # ... and the weights (>= 1) raise the loss
