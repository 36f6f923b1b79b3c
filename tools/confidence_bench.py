#!/usr/bin/env python3
"""Time of unetdc_label_confidence (csrc/confidence.hip) on a 1040 x 1388 label map -- the bright discs of
tools/quantify_e2e.py's synthetic micrographs labelled by unetdc_ccl_labels -- over a 512 x 512 probability plane (the flow's
geometry) and over a 1040 x 1388 one (the identity geometry of --tile), next to its yardstick unetdc_label_props without a grey
plane on the same map; and of unetdc_dihedral_mean_env_f32 next to unetdc_dihedral_mean_f32 at n = 8, S = 512, N = 8.
    python3 tools/confidence_bench.py [--calls N] [--windows W]
HIP events around N back-to-back calls, median (min .. max) of W windows."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from unet_dc_segmentation_amd import _lib
from unet_dc_segmentation_amd.droplets import _entropy_table

H, W = 1040, 1388


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, calls, windows):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return float(np.median(out)), f"{np.median(out):9.1f} us ({min(out):.1f} .. {max(out):.1f})"


def main():
    calls, windows = arg("--calls", 50), arg("--windows", 5)
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    cap = 1 << 14
    gray = bench.synthetic_micrograph(7)[..., 0]
    mask = torch.from_numpy((gray > 125).astype(np.uint8)).cuda()
    ws = torch.empty(lib.unetdc_ccl_labels_workspace(H, W), dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    area = torch.empty(cap, dtype=torch.int32, device="cuda")
    sums = torch.empty(2 + 14 + 10, cap, dtype=torch.int64, device="cuda")
    totals = torch.empty(8, dtype=torch.int64, device="cuda")
    label = torch.empty(H, W, dtype=torch.int32, device="cuda")
    maps = torch.empty(2, H, W, dtype=torch.uint8, device="cuda")
    table = _entropy_table(mask.device)
    _lib.call("unetdc_ccl_labels", mask.data_ptr(), H, W, 1, ws.data_ptr(), ws.numel(), count.data_ptr(), area.data_ptr(),
              sums[0].data_ptr(), sums[1].data_ptr(), None, label.data_ptr(), cap, s)
    k = int(count[0].item())
    rng = np.random.default_rng(0)

    def planes(ph, pw):
        """A probability plane that follows the mask (0.9 on droplets, 0.1 off, noise of 0.1) and an envelope around it."""
        yy = np.minimum(np.arange(ph) * H // ph, H - 1)[:, None]
        xx = np.minimum(np.arange(pw) * W // pw, W - 1)[None, :]
        p = np.where(gray[yy, xx] > 125, 0.85, 0.05).astype(np.float32) + rng.random((ph, pw), dtype=np.float32) * np.float32(0.1)
        d = rng.random((2, ph, pw), dtype=np.float32) * np.float32(0.1)
        return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in (p, p - d[0], p + d[1])]

    def props(lab=label):
        _lib.call("unetdc_label_props", lab.data_ptr(), None, H, W, sums[2].data_ptr(), cap, s)

    def confidence(pl, env, with_maps, lab=label):
        p, lo, hi = pl
        _lib.call("unetdc_label_confidence", lab.data_ptr(), cap, H, W, p.data_ptr(), lo.data_ptr() if env else None,
                  hi.data_ptr() if env else None, p.shape[0], p.shape[1], 0.3, 0.1, table.data_ptr(), sums[16].data_ptr(),
                  totals.data_ptr(), maps[0].data_ptr() if with_maps else None, maps[1].data_ptr() if with_maps and env else None, s)

    print(f"one MI355X; HIP events around {calls} back-to-back calls, median (min .. max) of {windows} windows, us per call")
    print(f"label map {H} x {W}: {k} droplets, foreground {float(mask.float().mean()):.3f}")
    base, text = timed(props, calls, windows)
    print(f"unetdc_label_props, no grey plane (yardstick)             : {text}")
    for ph, pw in ((512, 512), (H, W)):
        pl = planes(ph, pw)
        for env, with_maps in ((False, False), (True, False), (True, True)):
            t, text = timed(lambda: confidence(pl, env, with_maps), calls, windows)
            what = f"{ph} x {pw} plane{', envelope' if env else ''}{', maps' if with_maps else ''}"
            print(f"unetdc_label_confidence {what:34s}: {text}  = {t / base:.2f} x the yardstick")
    # no droplet pixel: every wave skips the segmented reductions, what is left is the per-pixel work and the image totals
    empty = torch.zeros_like(label)
    print(f"unetdc_label_props, empty map                             : {timed(lambda: props(empty), calls, windows)[1]}")
    for env in (False, True):
        text = timed(lambda: confidence(pl, env, False, empty), calls, windows)[1]
        print(f"unetdc_label_confidence empty map{', envelope' if env else '':25s}: {text}")
    n, S, N = 8, 512, 8
    items = torch.rand(n * N, S, S, device="cuda")
    outs = [torch.empty(n, S, S, device="cuda") for _ in range(3)]
    t0, text = timed(lambda: _lib.call("unetdc_dihedral_mean_f32", items.data_ptr(), n, S, N, outs[0].data_ptr(), s), calls, windows)
    print(f"unetdc_dihedral_mean_f32 n={n} S={S} N={N}                    : {text}  ({(4 * N + 4) * n * S * S / t0 * 1e-6:.2f} TB/s)")
    t1, text = timed(lambda: _lib.call("unetdc_dihedral_mean_env_f32", items.data_ptr(), n, S, N, *(o.data_ptr() for o in outs), s),
                     calls, windows)
    print(f"unetdc_dihedral_mean_env_f32 n={n} S={S} N={N}                : {text}  ({(4 * N + 12) * n * S * S / t1 * 1e-6:.2f} TB/s)"
          f"  = {t1 / t0:.2f} x the mean alone (bytes: {(4 * N + 12) / (4 * N + 4):.2f} x)")


if __name__ == "__main__":
    main()
