"""CPU: the separation weight map of the border-weighted loss.  utils/border_weights.py (the two-pass
form the kernels use) against the two restatements of tests/border_ref.py, the weighted PyTorch loss, the flags, and the
host-only part of the C ABI additions."""
import ctypes

import numpy as np
import pytest
import torch

from tests import border_ref as ref
from utils import border_weights as bw

RADII = (1, 3, 20, 64)


def noise_cases():
    for k, (h, w) in enumerate(((70, 131), (96, 128))):
        for j, dens in enumerate((0.02, 0.1, 0.3)):
            yield f"{h}x{w}_{dens}", ref.noise_mask(h, w, dens, 100 + 10 * k + j)


@pytest.mark.parametrize("R", RADII)
def test_two_pass_equals_brute_force_on_edge_cases(R):
    for name, m in ref.edge_cases(R):
        d1, d2 = bw.distance_planes(m, R)
        b1, b2 = ref.brute_planes(m, R)
        assert d1.dtype == np.int32 and d2.dtype == np.int32
        assert np.array_equal(d1, b1) and np.array_equal(d2, b2), (name, R)


def test_edge_cases_say_what_they_are_meant_to():
    """The masks of tests/border_ref.py exercise what their names claim (by the brute force, so for every implementation)."""
    R = 20
    cases = dict(ref.edge_cases(R))
    for name, m in cases.items():
        d1, d2 = ref.brute_planes(m, R)
        w = bw.weights_from_planes(d1, d2, 10.0, 5.0, R)
        if name.startswith(("empty", "full", "one_")):
            assert np.all(d2[m < 0.5] == ref.INF) and np.all(w == 1.0), name
    d1, d2 = ref.brute_planes(cases["two_pixels_gap_row"], R)
    assert (d1[0, 3], d2[0, 3]) == (1, 1)
    d1, d2 = ref.brute_planes(cases["diagonal_neighbours"], R)
    assert (d1[2, 4], d2[2, 4]) == (1, 1) and (d1[3, 3], d2[3, 3]) == (1, 1)       # two components, not one
    d1, d2 = ref.brute_planes(cases["behind_in_column"], R)
    assert (d1[5, 2], d2[5, 2]) == (4, 16)
    d1, d2 = ref.brute_planes(cases["u_shape"], R)
    assert d1[3, 4] == 4 and d2[3, 4] == ref.INF                                   # the other arm is the same droplet
    d1, d2 = ref.brute_planes(cases["u_shape_and_pixel"], R)
    assert (d1[3, 4], d2[3, 4]) == (4, 9)
    d1, d2 = ref.brute_planes(cases["second_at_R"], R)
    assert (d1[2, 1], d2[2, 1]) == (1, R * R)
    assert bw.weights_from_planes(d1, d2, 10.0, 5.0, R)[2, 1] > 1.0                # the cut-off is inclusive
    d1, d2 = ref.brute_planes(cases["second_past_R"], R)
    assert (d1[2, 1], d2[2, 1]) == (1, R * R + 1)
    assert bw.weights_from_planes(d1, d2, 10.0, 5.0, R)[2, 1] == 1.0


@pytest.mark.parametrize("R", RADII)
def test_two_pass_equals_brute_force_and_scipy_on_noise(R):
    cases = list(noise_cases())
    for name, m in (cases if R < 64 else [cases[0], cases[5]]):                    # (the brute force takes seconds at R = 64)
        d1, d2 = bw.distance_planes(m, R)
        b1, b2 = ref.brute_planes(m, R)
        assert np.array_equal(d1, b1) and np.array_equal(d2, b2), (name, R)
        s1, s2 = ref.scipy_planes(m)
        on, son = d2 <= R * R, s2 <= R * R
        assert np.array_equal(on, son), (name, R)                                  # the same set of weighted pixels
        assert np.array_equal(d1[on], s1[on]) and np.array_equal(d2[on], s2[on]), (name, R)


def test_batches_and_leading_dimensions_are_independent_images():
    ms = np.stack([m for _, m in noise_cases()][:3])[:, None]                      # [3, 1, 70, 131]
    w, d1, d2 = bw.border_weights_numpy(ms, 10.0, 5.0, None, planes=True)
    assert w.shape == ms.shape and w.dtype == np.float32
    for i in range(3):
        a1, a2 = bw.distance_planes(ms[i, 0], 20)
        assert np.array_equal(d1[i, 0], a1) and np.array_equal(d2[i, 0], a2)
    on, term = ref.weight64(d1, d2, 10.0, 5.0, 20)
    assert np.all(w[~on] == 1.0) and on.any()
    np.testing.assert_allclose(w[on], 1.0 + term[on], rtol=1e-7)


def test_parameter_checks():
    assert bw.default_radius(5.0) == 20 and bw.default_radius(0.1) == 1 and bw.default_radius(100.0) == 64
    assert bw.check_params(10, 5, None) == (10.0, 5.0, 20)
    for bad in ((-1, 5, None), (10, 0, None), (10, -1, 3), (10, 5, 0), (10, 5, 65), (float("nan"), 5, 3), (10, float("inf"), 3)):
        with pytest.raises(ValueError):
            bw.check_params(*bad)


def test_border_weights_of_cpu_tensors_is_the_numpy_path():
    from unet_dc_segmentation_amd.border import border_weights
    m = torch.from_numpy(ref.noise_mask(33, 47, 0.05, 7))[None, None]
    w, d1, d2 = border_weights(m, 10.0, planes=True)
    nw, n1, n2 = bw.border_weights_numpy(m.numpy(), 10.0, planes=True)
    assert torch.equal(w, torch.from_numpy(nw)) and torch.equal(d1, torch.from_numpy(n1)) and torch.equal(d2, torch.from_numpy(n2))
    out = torch.empty_like(w)
    assert border_weights(m, 10.0, out=out) is out and torch.equal(out, w)
    assert float(w.max()) > 1.0 and not w.requires_grad


@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_weighted_pytorch_loss(gamma):
    from utils import metrics_DC as M
    g = torch.Generator().manual_seed(5)
    p = torch.rand(2, 1, 24, 40, generator=g) * 0.98 + 0.01
    t = (torch.rand(2, 1, 24, 40, generator=g) < 0.3).float()
    a = p.clone().requires_grad_(True)
    b = p.clone().requires_grad_(True)
    plain = M.focal_dice_loss(a, t, alpha=0.75, gamma=gamma, ratio=0.4)
    ones = M.focal_dice_loss(b, t, alpha=0.75, gamma=gamma, ratio=0.4, weight=torch.ones_like(p))
    assert plain.item() == ones.item()                                             # weight = 1 is the unweighted loss
    plain.backward()
    ones.backward()
    assert torch.equal(a.grad, b.grad)
    w = 1.0 + 10.0 * torch.rand(2, 1, 24, 40, generator=g)
    w.requires_grad_(True)                                                         # even so: no gradient flows into it
    c = p.clone().requires_grad_(True)
    got = M.focal_dice_loss(c, t, alpha=0.75, gamma=gamma, ratio=0.4, weight=w)
    focal = M.FocalLoss(alpha=0.75, gamma=gamma, reduction="none")(p, t)
    want = 0.4 * (w.detach() * focal).sum() / p.numel() + 0.6 * M.dice_loss(p, t)
    assert abs(got.item() - want.item()) < 1e-6
    got.backward()
    assert w.grad is None and c.grad is not None
    with pytest.raises(ValueError):
        M.focal_dice_loss(p, t, weight=torch.ones(2, 1, 24, 41))


def test_parser_accepts_and_refuses():
    import train_DC_focal as T
    p = T.build_parser()
    a = p.parse_args([])
    assert a.border_weight is None and a.border_sigma is None and a.border_radius is None
    assert T.check_border_flags(p, a) is None
    assert T.check_border_flags(p, p.parse_args(["--border_weight"])) == (10.0, 5.0, 20)
    assert T.check_border_flags(p, p.parse_args(["--border_weight", "4", "--border_sigma", "2"])) == (4.0, 2.0, 8)
    assert T.check_border_flags(p, p.parse_args(["--border_weight", "--border_radius", "7"])) == (10.0, 5.0, 7)
    for bad in (["--border_weight", "--loss", "bce_dice"], ["--border_sigma", "3"], ["--border_radius", "3"],
                ["--border_weight", "-1"], ["--border_weight", "--border_sigma", "0"], ["--border_weight", "--border_radius", "65"],
                ["--border_weight", "--border_radius", "0"]):
        args = p.parse_args(bad)
        with pytest.raises(SystemExit) as e:
            T.check_border_flags(p, args)
        assert e.value.code == 2, bad                                              # a parser error
    # train.py's parser defaults to bce_dice: the flag is an error there unless the loss is chosen too
    q = T.build_parser(arch="unet", epochs=50, ckpt="x.pth", loss="bce_dice")
    with pytest.raises(SystemExit):
        T.check_border_flags(q, q.parse_args(["--border_weight"]))
    assert T.check_border_flags(q, q.parse_args(["--border_weight", "--loss", "focal_dice"])) == (10.0, 5.0, 20)
    with pytest.raises(SystemExit) as e:
        T.main(["--synthetic", "--border_weight", "--loss", "bce_dice", "--device", "cpu"])
    assert e.value.code == 2


def test_training_on_the_cpu_with_the_flag(tmp_path):
    """The host path end to end: one tiny epoch on the CPU with and without --border_weight."""
    import train_DC_focal as T
    common = ["--synthetic", "--synthetic_len", "10", "--batch", "2", "--img_size", "64", "--epochs", "1", "--steps", "1",
              "--in_channels", "1", "--device", "cpu", "--workers", "0", "--no_test_eval", "--ckpt_path", str(tmp_path / "m.pth")]
    plain = T.main(common)
    weighted = T.main(common + ["--border_weight"])
    assert np.isfinite(weighted[0]["train_loss"]) and weighted[0]["train_loss"] != plain[0]["train_loss"]


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_abi_workspace_query(lib):
    assert lib.unetdc_version() == 2
    assert lib.unetdc_border_weights_workspace(8, 512, 512, 20) == 8 * 512 * 512 * 14 + 64
    assert lib.unetdc_border_weights_workspace(1, 1, 1, 1) > 0
    assert lib.unetdc_border_weights_workspace(1, 16384, 16384, 64) > 0
    for n, h, w, r in ((0, 8, 8, 3), (-1, 8, 8, 3), (65536, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 16385, 8, 3), (1, 8, 16385, 3),
                       (1, 8, 8, 0), (1, 8, 8, 65), (1, 8, 8, -1)):
        assert lib.unetdc_border_weights_workspace(n, h, w, r) == 0, (n, h, w, r)


def test_abi_refuses_before_any_hip_call(lib):
    """Null and range arguments come back as UNETDC_EINVAL (EWORKSPACE for a short workspace) with a message, before any HIP
    call: host memory stands in for the device pointers."""
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    a += (-a) % 16
    ok = dict(target=a, n=1, h=4, w=4, w0=10.0, sigma=5.0, radius=3, out=a, d1=None, d2=None, ws=a, nbytes=2048)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.unetdc_border_weights(v["target"], v["n"], v["h"], v["w"], v["w0"], v["sigma"], v["radius"], v["out"], v["d1"],
                                         v["d2"], v["ws"], v["nbytes"], None)

    for kw in (dict(target=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == -1 and b"null" in lib.unetdc_last_error(), kw
    for kw in (dict(n=0), dict(h=0), dict(w=0), dict(h=16385), dict(w=16385), dict(n=65536), dict(radius=0), dict(radius=65)):
        assert call(**kw) == -1 and b"geometry" in lib.unetdc_last_error(), kw
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(w0=-1.0),
               dict(w0=float("nan"))):
        assert call(**kw) == -1 and b"sigma" in lib.unetdc_last_error(), kw
    assert call(ws=a + 2) == -1 and b"aligned" in lib.unetdc_last_error()
    assert call(nbytes=16 * 14 + 63) == -3 and b"workspace too small" in lib.unetdc_last_error()
    # the weighted loss: a null weight, then the checks of the unweighted launcher
    rc = lib.unetdc_focal_dice_loss_w_fwd(a, a, None, a, a, a, 2048, 1, 16, 1.0, 2.0, 0.3, 1e-7, None)
    assert rc == -1 and b"null weight" in lib.unetdc_last_error()
    rc = lib.unetdc_focal_dice_loss_w_bwd(a, a, None, a, a, a, 1, 16, 1.0, 2.0, 0.3, None)
    assert rc == -1 and b"null weight" in lib.unetdc_last_error()
    rc = lib.unetdc_focal_dice_loss_w_fwd(None, a, a, a, a, a, 2048, 1, 16, 1.0, 2.0, 0.3, 1e-7, None)
    assert rc == -1 and b"null pointer" in lib.unetdc_last_error()
    rc = lib.unetdc_focal_dice_loss_w_fwd(a, a, a, a, a, a, 2048, 0, 16, 1.0, 2.0, 0.3, 1e-7, None)
    assert rc == -1 and b"bad shape" in lib.unetdc_last_error()
    rc = lib.unetdc_focal_dice_loss_w_fwd(a, a, a, a, a, a, 8, 1, 16, 1.0, 2.0, 0.3, 1e-7, None)
    assert rc == -3 and b"workspace too small" in lib.unetdc_last_error()
    rc = lib.unetdc_focal_dice_loss_w_bwd(a, a, a, a, a, None, 1, 16, 1.0, 2.0, 0.3, None)
    assert rc == -1 and b"null pointer" in lib.unetdc_last_error()
