#!/usr/bin/env python3
"""Time of unetdc_label_hull (csrc/hull.hip) on a 1040 x 1388 label map -- the bright discs of
tools/quantify_e2e.py's synthetic micrographs labelled by unetdc_ccl_labels -- next to its yardstick unetdc_label_props without a
grey plane on the same map; on an empty map; and the tall-label case: one label that spans the whole height of the plane (a
lens 1040 rows tall), alone and with the droplets beside it.
    python3 tools/hull_bench.py [--calls N] [--windows W] [--once]
HIP events around N back-to-back calls, median (min .. max) of W windows.  --once: every case once, for a kernel trace."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from unet_dc_segmentation_amd import _lib
from unet_dc_segmentation_amd.droplets import ROWS_PER_DROPLET

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
    once = "--once" in sys.argv
    calls, windows = (1, 1) if once else (arg("--calls", 50), arg("--windows", 5))
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    cap = 1 << 14
    room = min(ROWS_PER_DROPLET * cap, H * W)                # what droplets.py gives the first launch
    gray = bench.synthetic_micrograph(7)[..., 0]
    mask = torch.from_numpy((gray > 125).astype(np.uint8)).cuda()
    ws = torch.empty(max(lib.unetdc_ccl_labels_workspace(H, W), lib.unetdc_label_hull_workspace(H, W, cap, room)), dtype=torch.uint8,
                     device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    area = torch.empty(cap, dtype=torch.int32, device="cuda")
    sums = torch.empty(2 + 14 + 5, cap, dtype=torch.int64, device="cuda")
    label = torch.empty(H, W, dtype=torch.int32, device="cuda")
    _lib.call("unetdc_ccl_labels", mask.data_ptr(), H, W, 1, ws.data_ptr(), ws.numel(), count.data_ptr(), area.data_ptr(),
              sums[0].data_ptr(), sums[1].data_ptr(), None, label.data_ptr(), cap, s)
    k = int(count[0].item())
    y = np.arange(H)
    bend = np.rint(200 * ((y - H / 2) / (H / 2)) ** 2).astype(np.int64)
    lens = np.zeros((H, W), np.int32)
    for r in range(H):
        lens[r, 500 + bend[r]:900 - bend[r]] = 1
    tall_alone = torch.from_numpy(lens).cuda()
    both = label.clone()
    both[tall_alone > 0] = k + 1                             # the lens over the droplets, as one more label

    def props(lab=label):
        _lib.call("unetdc_label_props", lab.data_ptr(), None, H, W, sums[2].data_ptr(), cap, s)

    def hull(lab=label, max_out=cap):
        _lib.call("unetdc_label_hull", lab.data_ptr(), max_out, H, W, ws.data_ptr(), ws.numel(), sums[16].data_ptr(), count[1:].data_ptr(),
                  room, s)

    print(f"one MI355X; HIP events around {calls} back-to-back calls, median (min .. max) of {windows} windows, us per call")
    print(f"label map {H} x {W}: {k} droplets, foreground {float(mask.float().mean()):.3f}; capacity {cap}, row room {room}")
    base, text = timed(props, calls, windows)
    print(f"unetdc_label_props, no grey plane (yardstick)       : {text}")
    for what, lab, mo in (("synthetic droplets", label, cap), ("synthetic droplets, capacity = droplets", label, max(k, 1)),
                          ("empty map", torch.zeros_like(label), cap), ("one label 1040 rows tall, alone", tall_alone, cap),
                          ("droplets + the tall label", both, cap)):
        t, text = timed(lambda: hull(lab, mo), calls, windows)
        rows = int(count[1].item())
        nv = int(sums[16:].reshape(-1)[4 * mo:5 * mo].max().item())       # row 4 of out[5][max_out]
        print(f"unetdc_label_hull {what:34s}: {text}  = {t / base:.2f} x the yardstick   (rows {rows}, most vertices {nv})")


if __name__ == "__main__":
    main()
