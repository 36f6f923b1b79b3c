"""CPU: the C-ABI shared library loads and exports every symbol include/unetdc_hip.h declares
(no compute calls -- there is no GPU here), and the ctypes table mirrors the header."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unetdc_hip.h")


def declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(unetdc_[a-z0-9_A-Z]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from unet_dc_segmentation_amd import build
    build.build(force=False, verbose=False)            # hipcc cross-compiles gfx950 without a GPU
    from unet_dc_segmentation_amd import _lib
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    names = declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "unet_dc_segmentation_amd",
                                                                     "libunetdc_hip.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (unetdc_\w+)", out))
    assert set(names) <= exported, set(names) - exported


def test_ctypes_table_matches_header(lib):
    from unet_dc_segmentation_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))


def test_host_only_queries_and_error_reporting(lib):
    assert lib.unetdc_version() == 2
    # pure host-side planning queries (no device needed)
    assert lib.unetdc_conv3x3_stats_rows(8 * 512 * 512, 64) == 8192
    assert lib.unetdc_conv3x3_stats_rows(8 * 32 * 32, 1024) == 32
    assert lib.unetdc_conv3x3_wgrad_workspace(8, 512, 512, 64, 64, 1) > 0
    assert lib.unetdc_bn_relu_bwd_workspace(8, 512, 512, 64, 1, 1) > 0
    # argument validation happens before any HIP call: bad shapes give a negative code + message
    rc = lib.unetdc_conv3x3_fwd(None, 64, None, None, None, None, None, 64, None, None, 1, 8, 8, 64, 64, 1, 0, None)
    assert rc == -1 and b"null" in lib.unetdc_last_error()
    rc = lib.unetdc_conv3x3_fwd(None, 64, None, None, None, None, None, 64, None, None, 0, 8, 8, 64, 64, 1, 0, None)
    assert rc == -1 and b"geometry" in lib.unetdc_last_error()


def test_wgrad_workspace_and_bnin_answers_are_the_recorded_ones(lib, golden_dir):
    """The host-only planning answers of the 3x3 weight gradient, against tests/golden/wgrad_abi_answers.json: every
    unetdc_conv3x3_wgrad_workspace and unetdc_conv3x3_bnin_supported value over fp32 / bf16, n in {1, 3, 5, 8}, five image
    sizes from 64^2 to 1024^2, the 13 channel pairs of the networks and d in {1, 2, 4, 8}.  The table was recorded from the
    library of the commit BEFORE the tap-fused route got its single plan (plan_wgrad_fused); a change of the planning code
    must reproduce it, or say why an answer moves."""
    import json
    t = json.load(open(os.path.join(golden_dir, "wgrad_abi_answers.json")))
    assert t["dtypes"] == [0, 1] and t["n"] == [1, 3, 5, 8] and t["d"] == [1, 2, 4, 8]
    assert [64, 64] in t["hw"] and [96, 128] in t["hw"] and [1024, 1024] in t["hw"] and len(t["hw"]) == 5 and len(t["pairs"]) == 13
    checked, bad = 0, []
    for a, dt in enumerate(t["dtypes"]):
        for b, n in enumerate(t["n"]):
            for c, (h, w) in enumerate(t["hw"]):
                for e, (cin, cout) in enumerate(t["pairs"]):
                    got = lib.unetdc_conv3x3_wgrad_workspace(n, h, w, cin, cout, dt)
                    want = t["workspace"][a][b][c][e]
                    checked += 1
                    if got != want:
                        bad.append(("workspace", dt, n, h, w, cin, cout, got, want))
                    for f, d in enumerate(t["d"]):
                        got = lib.unetdc_conv3x3_bnin_supported(n, h, w, cin, cout, d, dt)
                        want = t["bnin_supported"][a][b][c][e][f]
                        checked += 1
                        if got != want:
                            bad.append(("bnin_supported", dt, n, h, w, cin, cout, d, got, want))
    assert checked == 520 + 2080
    assert not bad, bad[:10]


def test_partial_buffer_sizing_answers_are_the_recorded_ones(lib, golden_dir):
    """The host-only sizing answers of the HBM-bound operators, against tests/golden/elementwise_abi_answers.json: recorded from
    the library of the commit BEFORE each operator got its single plan (plan_bn_bwd, plan_head, plan_channel_sum) and the
    spare-row helpers.  fp32 / bf16, n in {1, 3, 5, 8}, six image sizes from 16^2 to 1024^2: unetdc_bn_relu_bwd_workspace over
    seven widths, pooled or not; unetdc_head_bwd_workspace over six widths and OC in {1, 2, 3}; unetdc_channel_sum_workspace,
    unetdc_conv3x3_dgrad_colsum_workspace and unetdc_conv3x3_stats_rows over the pixel counts and widths of that grid."""
    import json
    t = json.load(open(os.path.join(golden_dir, "elementwise_abi_answers.json")))
    assert t["dtypes"] == [0, 1] and t["n"] == [1, 3, 5, 8] and t["pooled"] == [0, 1] and t["oc"] == [1, 2, 3]
    assert t["hw"] == [[16, 16], [24, 40], [64, 64], [96, 128], [512, 512], [1024, 1024]]
    assert t["bn_c"] == [8, 64, 128, 256, 512, 1024, 2048] and t["head_c"] == [8, 16, 32, 64, 128, 256]
    checked, bad = 0, []

    def check(what, got, want, *args):
        nonlocal checked
        checked += 1
        if got != want:
            bad.append((what, *args, got, want))

    for b, n in enumerate(t["n"]):
        for c, (h, w) in enumerate(t["hw"]):
            for a, dt in enumerate(t["dtypes"]):
                for e, ch in enumerate(t["bn_c"]):
                    for f, pooled in enumerate(t["pooled"]):
                        check("bn_relu_bwd_workspace", lib.unetdc_bn_relu_bwd_workspace(n, h, w, ch, pooled, dt),
                              t["bn_relu_bwd_workspace"][a][b][c][e][f], n, h, w, ch, pooled, dt)
                for e, ch in enumerate(t["head_c"]):
                    for f, oc in enumerate(t["oc"]):
                        check("head_bwd_workspace", lib.unetdc_head_bwd_workspace(n, h, w, ch, oc, dt),
                              t["head_bwd_workspace"][a][b][c][e][f], n, h, w, ch, oc, dt)
            for e, ch in enumerate(t["bn_c"]):
                check("channel_sum_workspace", lib.unetdc_channel_sum_workspace(n * h * w, ch), t["channel_sum_workspace"][b][c][e],
                      n * h * w, ch)
                check("dgrad_colsum_workspace", lib.unetdc_conv3x3_dgrad_colsum_workspace(n, h, w, ch),
                      t["dgrad_colsum_workspace"][b][c][e], n, h, w, ch)
                check("stats_rows", lib.unetdc_conv3x3_stats_rows(n * h * w, ch), t["stats_rows"][b][c][e], n * h * w, ch)
    assert checked == 672 + 864 + 3 * 168
    assert not bad, bad[:10]


def test_sizing_queries_answer_zero_for_widths_the_launchers_refuse(lib):
    """A width the launcher would refuse (no multiple of the 16-byte chunk, zero, a head width outside the powers of two up to
    64 chunks) gets 0 bytes, like every other *_workspace query -- not a division by zero in the host process."""
    BF16 = 1
    assert lib.unetdc_bn_relu_bwd_workspace(1, 8, 8, 4, 0, BF16) == 0
    assert lib.unetdc_bn_relu_bwd_workspace(1, 8, 8, 0, 0, BF16) == 0
    assert lib.unetdc_head_bwd_workspace(1, 8, 8, 4, 1, BF16) == 0
    assert lib.unetdc_head_bwd_workspace(1, 8, 8, 4096, 1, BF16) == 0
    # the launchers refuse the same widths before any arithmetic on them, and before any HIP call (host memory stands in)
    import ctypes
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    for c, msg in ((0, b"unsupported"), (4, b"chunk aligned")):
        rc = lib.unetdc_bn_relu_bwd(a, c, None, 0, a, c, a, a, a, a, a, a, c, a, a, a, a, 64, None, 0, 1, 8, 8, c, BF16, None)
        assert rc == -1 and msg in lib.unetdc_last_error(), (c, rc, lib.unetdc_last_error())
    for c in (4, 4096):
        rc = lib.unetdc_head_bwd(a, a, a, 8 * c, a, a, 8 * c, a, a, a, 64, 1, 8, 8, c, 1, BF16, None)
        assert rc == -1 and b"unsupported" in lib.unetdc_last_error(), (c, rc, lib.unetdc_last_error())
    rc = lib.unetdc_channel_sum(a, 0, a, a, 64, 16, 0, BF16, None)
    assert rc == -1 and b"unsupported" in lib.unetdc_last_error(), (rc, lib.unetdc_last_error())


def test_no_kernel_carries_packed_fp32(lib):
    """Build guard (widened in round 3 to EVERY kernel of the library): the packed-fp32 (SLP-vectorised) build
    of the fused BatchNorm-backward epilogue was not run-to-run deterministic on MI355X and the cause is not identified
    (DESIGN.md section 7); the library is built with -fno-slp-vectorize.  Disassemble the gfx950 code objects of the library
    and fail if a toolchain or flag change brings v_pk_{add,mul,fma}_f32 back anywhere -- convolutions, BatchNorm, head,
    optimizer, elementwise, first layer (the GPU-side determinism test only proves that one build is stable)."""
    from unet_dc_segmentation_amd import build
    rep = build.packed_f32_report()
    assert len(rep) >= 100 and sum(1 for k in rep if re.search(r"igemm|wgrad_(dma|ring|fused|rect)|bn_|head_", k)) >= 20, sorted(rep)
    bad = {k: v for k, v in rep.items() if v}
    assert not bad, bad
