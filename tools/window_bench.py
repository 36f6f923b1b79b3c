#!/usr/bin/env python3
"""Time of the deep-image window (csrc/window.hip) on a 1040 x 1388 16-bit frame: the ranks call (five
requests, as the flow issues it), the window to 8 bits and the plane maximum, next to two yardsticks that read an image of the
same pixel count once -- unetdc_label_props without a grey plane and unetdc_thresh_sweep (nearest rule).  Three frames: a smooth
12-bit micrograph (few occupied high bytes: the case where LDS atomics meet on one bin), uniform noise over all 16 bits, and
one value everywhere.
    python3 tools/window_bench.py [--calls N] [--windows W] [--once]
HIP events around N back-to-back calls, median (min .. max) of W windows.  --once: every case once, for a kernel trace."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from unet_dc_segmentation_amd import _lib
from unet_dc_segmentation_amd import window as wd
from utils import intensity_window as iw

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
    return f"{np.median(out):9.1f} us ({min(out):.1f} .. {max(out):.1f})"


def deep_micrograph(seed):
    """bench.synthetic_micrograph as a 12-bit camera would have recorded it: grey x 16 plus four bits of noise, uint16 [H, W]."""
    g = bench.synthetic_micrograph(seed)[..., 0].astype(np.uint16)
    return g * 16 + np.random.default_rng(seed).integers(0, 16, g.shape).astype(np.uint16)


def main():
    once = "--once" in sys.argv
    calls, windows = (1, 1) if once else (arg("--calls", 50), arg("--windows", 5))
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    spec = iw.WindowSpec(1000, 999000)
    ppm = np.asarray(spec.ppm, np.int32)
    print(f"one MI355X; HIP events around {calls} back-to-back calls, median (min .. max) of {windows} windows, us per call")
    label = torch.from_numpy((bench.synthetic_micrograph(7)[..., 0] > 125).astype(np.int32)).cuda()
    sums = torch.empty(14, 1 << 14, dtype=torch.int64, device="cuda")
    probs = torch.rand(1, H, W, device="cuda")
    gt = (label > 0).to(torch.uint8)
    hist = torch.zeros(2, 257, dtype=torch.int64, device="cuda")
    print("yardsticks on 1040 x 1388:")
    print("  unetdc_label_props, no grey plane                   :",
          timed(lambda: _lib.call("unetdc_label_props", label.data_ptr(), None, H, W, sums.data_ptr(), 1 << 14, s), calls, windows))
    print("  unetdc_thresh_sweep, K = 256, nearest               :",
          timed(lambda: _lib.call("unetdc_thresh_sweep", probs.data_ptr(), 1, H, W, gt.data_ptr(), H, W, None, None, None, None, 256,
                                  hist.data_ptr(), s), calls, windows))
    rng = np.random.default_rng(0)
    frames = {"12-bit micrograph": deep_micrograph(7), "uniform 16-bit noise": rng.integers(0, 65536, (H, W)).astype(np.uint16),
              "one value": np.full((H, W), 1234, np.uint16)}
    for c in (1, 3):
        for name, grey in frames.items():
            arr = np.ascontiguousarray(np.repeat(grey[:, :, None], c, axis=2))
            t = wd.upload_u16(arr)
            nq = len(ppm)
            nbytes = lib.unetdc_u16_ranks_workspace(H, W, c, nq)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            out = torch.empty(3, c, nq, dtype=torch.int32, device="cuda")
            dst = torch.empty(H, W, 3, dtype=torch.uint8, device="cuda")

            def ranks():
                _lib.call("unetdc_u16_ranks", t.data_ptr(), H, W, c, ppm.ctypes.data, nq, ws.data_ptr(), nbytes, out[0].data_ptr(),
                          out[1].data_ptr(), out[2].data_ptr(), s)

            ranks()
            levels = torch.stack((out[0][:, 1], out[0][:, 3]), dim=1).contiguous()
            want = np.stack(iw.ranks_numpy(arr, spec.ppm))
            assert np.array_equal(out.cpu().numpy(), want), "the device ranks differ from ranks_numpy"
            occupied = len(np.unique(grey >> 8))
            print(f"{name}, c = {c} ({occupied} occupied high bytes; levels {levels[0].tolist()}):")
            print("  unetdc_u16_ranks, 5 requests (zero, A, select, B, select):", timed(ranks, calls, windows))
            print("  unetdc_window_u16_to_u8 -> 3 channels                :",
                  timed(lambda: _lib.call("unetdc_window_u16_to_u8", t.data_ptr(), H, W, c, levels.data_ptr(), dst.data_ptr(), 3, s),
                        calls, windows))
    planes = wd.upload_u16(np.stack([frames["12-bit micrograph"]] * 8))
    pm = torch.empty(H, W, dtype=torch.int16, device="cuda")
    for p in (2, 8):
        print(f"  unetdc_planes_max_u16, {p} planes                      :",
              timed(lambda: _lib.call("unetdc_planes_max_u16", planes.data_ptr(), p, H, W, pm.data_ptr(), s), calls, windows))
    host = frames["12-bit micrograph"][:, :, None]
    import time
    t0 = time.perf_counter()
    iw.deep_to_u8_numpy(host, spec)
    print(f"  deep_to_u8_numpy on this host (the CPU path), wall clock: {(time.perf_counter() - t0) * 1e6:9.1f} us")
    t0 = time.perf_counter()
    for _ in range(10):
        u8, _ = wd.deep_to_u8_device(host, spec)
    torch.cuda.synchronize()
    print(f"  deep_to_u8_device incl. the 2.9 MB upload, wall clock    : {(time.perf_counter() - t0) * 1e5:9.1f} us")


if __name__ == "__main__":
    main()
