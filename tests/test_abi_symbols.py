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


IMAGE_SIZES = [(1, 1), (1, 64), (37, 53), (64, 64), (96, 130), (300, 401), (1040, 1388), (16384, 16384)]
IMAGE_LIMITS = [0, 1, 33, 2 ** 14, 2 ** 27]       # max_label, max_pairs


def image_abi_cases():
    """{query: [argument tuple, ...]}: the geometries every image-side launcher accepts, then the refusals that
    include/unetdc_hip.h documents (a non-positive or 16385-pixel side, h * w >= 2^30, radius 0 and 65, a negative limit)."""
    bad_sides = [(0, 5), (5, 0), (-1, 5)]
    too_long = [(16385, 5), (5, 16385)]
    c = {}
    c["unetdc_ccl_workspace"] = list(IMAGE_SIZES)
    c["unetdc_ccl_labels_workspace"] = IMAGE_SIZES + bad_sides
    c["unetdc_split_workspace"] = IMAGE_SIZES + bad_sides
    c["unetdc_mask_clean_workspace"] = IMAGE_SIZES + bad_sides + too_long
    c["unetdc_label_overlap_workspace"] = ([(h, w, mp) for h, w in IMAGE_SIZES for mp in IMAGE_LIMITS] +
                                           [(h, w, 33) for h, w in bad_sides + too_long] + [(64, 64, -1)])
    c["unetdc_label_neighbors_workspace"] = ([(h, w, ml, mp) for h, w in IMAGE_SIZES for ml in IMAGE_LIMITS for mp in IMAGE_LIMITS] +
                                             [(h, w, 33, 33) for h, w in bad_sides + too_long] + [(64, 64, -1, 33), (64, 64, 33, -1)])
    c["unetdc_border_weights_workspace"] = ([(n, h, w, r) for n in (1, 3, 8) for h, w in IMAGE_SIZES for r in (1, 64)] +
                                            [(1, h, w, 5) for h, w in bad_sides + too_long] +
                                            [(1, 64, 64, 0), (1, 64, 64, 65), (0, 64, 64, 5)])
    c["unetdc_density_workspace"] = ([s for s in IMAGE_SIZES if min(s) >= 2] + [(1, 1), (1, 64)] + bad_sides +
                                     [(32768, 32768)])
    c["unetdc_rolling_ball_workspace"] = [(h, w, cn) for h, w in IMAGE_SIZES for cn in (1, 2, 3, 4)]
    c["unetdc_elastic_fields_workspace"] = ([(n, h, w, s) for n in (1, 3, 8) for h, w in IMAGE_SIZES if max(h, w) <= 1024
                                             for s in (0.5, 8.0)] +
                                            [(-1, 64, 64, 8.0), (1, 0, 64, 8.0), (1, 64, 0, 8.0), (1, 64, 64, 0.0),
                                             (1, 64, 64, -1.0), (1, 64, 64, 300.0)])
    c["unetdc_focal_dice_loss_workspace"] = [(n, h * w) for n in (1, 3, 8) for h, w in IMAGE_SIZES]
    return c


def test_image_workspace_answers_are_the_recorded_ones(lib, golden_dir):
    """The eleven host-only workspace queries of the image-side stages, against tests/golden/image_abi_answers.json: recorded
    from the library of the commit BEFORE each stage got its single layout function (csrc/workspace.h), over image_abi_cases().
    A refused geometry answers 0, for unetdc_elastic_fields_workspace -1."""
    import json
    t = json.load(open(os.path.join(golden_dir, "image_abi_answers.json")))
    cases = image_abi_cases()
    assert sorted(t) == sorted(cases) and len(cases) == 11
    checked, bad = 0, []
    for name, rows in cases.items():
        assert [tuple(r[:-1]) for r in t[name]] == rows, name
        for args, rec in zip(rows, t[name]):
            got = getattr(lib, name)(*args)
            checked += 1
            if got != rec[-1]:
                bad.append((name, args, got, rec[-1]))
    assert checked == 8 + 11 + 11 + 13 + 46 + 207 + 56 + 12 + 32 + 42 + 24
    assert not bad, bad[:10]
    refused = {n: [r[-1] for r in t[n] if min(r[:2]) <= 0] for n in t if n not in ("unetdc_ccl_workspace", "unetdc_rolling_ball_workspace",
                                                                                    "unetdc_focal_dice_loss_workspace")}
    assert all(v and set(v) == {-1 if n == "unetdc_elastic_fields_workspace" else 0} for n, v in refused.items()), refused


def test_ccl_stats_and_rolling_ball_refuse_a_workspace_one_byte_short(lib):
    """Both check the workspace size before any HIP call (host memory stands in for device memory): one byte less than their
    query names is UNETDC_EWORKSPACE, and the message names the stage."""
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    need = lib.unetdc_ccl_workspace(37, 53)
    rc = lib.unetdc_ccl_stats(a, 37, 53, 1, a, need - 1, a, a, a, a, a, 8, None)
    err = lib.unetdc_last_error()
    assert rc == -3 and err.startswith(b"ccl_stats") and b"workspace too small" in err, (rc, err)
    need = lib.unetdc_rolling_ball_workspace(37, 53, 3)
    rc = lib.unetdc_rolling_ball_u8(a, a + 64, 37, 53, 3, 50, a, need - 1, None)
    err = lib.unetdc_last_error()
    assert rc == -3 and err.startswith(b"rolling_ball") and b"workspace too small" in err, (rc, err)
    # the size check comes before the 16-byte alignment check
    rc = lib.unetdc_rolling_ball_u8(a + 1, a + 64, 37, 53, 3, 50, a, need - 1, None)
    assert rc == -3, (rc, lib.unetdc_last_error())
    rc = lib.unetdc_rolling_ball_u8(a + 1, a + 64, 37, 53, 3, 50, a, need, None)
    assert rc == -1 and b"aligned" in lib.unetdc_last_error(), (rc, lib.unetdc_last_error())


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
