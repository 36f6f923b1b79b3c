#!/usr/bin/env python3
"""Time of unetdc_droplet_points + unetdc_ripley_counts (csrc/spatial.hip) on a 1040 x 1388 image:
N in {250, 3 000, 16 384} uniform points, R = 64, S in {0, 99} simulated patterns, without a window and with one (a disc that
leaves the corners out), next to its yardsticks: unetdc_ccl_labels + unetdc_label_props on a synthetic micrograph of
tools/quantify_e2e.py, and ripley_counts_numpy on the host on the same inputs.
    python3 tools/spatial_bench.py [--calls N] [--windows W] [--once]
HIP events around N back-to-back calls, median (min .. max) of W windows.  --once: one call per case and no host yardstick
(for a kernel trace).  The host path at N = 16 384 with S = 99 is not run: (1 + S) times its S = 0 time is printed instead."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from unet_dc_segmentation_amd import _lib
from utils import spatial_stats as ss

H, W, R = 1040, 1388, 64


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
    return f"{np.median(out):10.1f} us ({min(out):.1f} .. {max(out):.1f})", float(np.median(out))


def main():
    once = "--once" in sys.argv
    calls, windows = (1, 1) if once else (arg("--calls", 10), arg("--windows", 5))
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    cap = 1 << 14
    mask = torch.from_numpy((bench.synthetic_micrograph(7)[..., 0] > 125).astype(np.uint8)).cuda()
    ws = torch.empty(max(lib.unetdc_ccl_labels_workspace(H, W), lib.unetdc_ripley_workspace(H, W, cap, R, 99)), dtype=torch.uint8,
                     device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    area = torch.empty(cap, dtype=torch.int32, device="cuda")
    sums = torch.empty(2 + 14, cap, dtype=torch.int64, device="cuda")
    label = torch.empty(H, W, dtype=torch.int32, device="cuda")

    def label_it():
        _lib.call("unetdc_ccl_labels", mask.data_ptr(), H, W, 1, ws.data_ptr(), ws.numel(), count.data_ptr(), area.data_ptr(),
                  sums[0].data_ptr(), sums[1].data_ptr(), None, label.data_ptr(), cap, s)
        _lib.call("unetdc_label_props", label.data_ptr(), None, H, W, sums[2].data_ptr(), cap, s)

    print(f"one MI355X; HIP events around {calls} back-to-back calls, median (min .. max) of {windows} windows, us per call")
    print(f"image {H} x {W}, R = {R}")
    print(f"unetdc_ccl_labels + unetdc_label_props (yardstick, {int((label_it(), count.item())[1])} droplets): {timed(label_it, calls, windows)[0]}")
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (((yy - H / 2) / (H / 2)) ** 2 + ((xx - W / 2) / (W / 2)) ** 2 <= 1.0).astype(np.uint8)
    py_d, px_d = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    for kind, window in (("no window", None), ("disc window", disc)):
        win = None if window is None else torch.from_numpy(window).cuda()
        wptr = None if win is None else win.data_ptr()
        for N in (250, 3000, 16384):
            y, x = ss.simulated_points(N, 0, N, H, W, window)
            one = torch.ones(N, dtype=torch.int32, device="cuda")
            sy, sx = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()          # area 1: the sums are the pixels
            cnt = torch.tensor([N], dtype=torch.int32, device="cuda")
            host0 = None
            for S in (0, 99):
                rows = (1 + S) * (R + 1)
                n = torch.empty(rows, dtype=torch.int32, device="cuda")
                pairs, pairs_all = (torch.empty(rows, dtype=torch.int64, device="cuda") for _ in range(2))

                def op():
                    _lib.call("unetdc_droplet_points", cnt.data_ptr(), one.data_ptr(), sy.data_ptr(), sx.data_ptr(), cap, wptr, H, W,
                              py_d.data_ptr(), px_d.data_ptr(), info.data_ptr(), s)
                    _lib.call("unetdc_ripley_counts", py_d.data_ptr(), px_d.data_ptr(), info.data_ptr(), cap, wptr, H, W, R, S, 1,
                              ws.data_ptr(), ws.numel(), n.data_ptr(), pairs.data_ptr(), pairs_all.data_ptr(), s)

                text, us = timed(op, calls, windows)
                rate = (1 + S) * N * N / us * 1e-3                                    # pair distances per nanosecond
                line = f"{kind:11s} N={N:6d} S={S:2d}: {text}; {rate:7.1f} pairs/ns; pairs[R] = {int(pairs[R].item())}"
                if not once:
                    if S == 0 or N <= 3000:
                        t0 = time.perf_counter()
                        want = ss.ripley_counts_numpy(y, x, H, W, R, S, 1, window)
                        ms = (time.perf_counter() - t0) * 1e3
                        host0 = ms if S == 0 else host0
                        ok = np.array_equal(want[1].ravel(), pairs.cpu().numpy()) and np.array_equal(want[0].ravel(), n.cpu().numpy())
                        line += f"; host {ms:9.1f} ms, equal: {ok}"
                    else:
                        line += f"; host about {(1 + S) * host0:9.1f} ms ((1 + S) x its S = 0 time, not run)"
                print(line, flush=True)


if __name__ == "__main__":
    main()
