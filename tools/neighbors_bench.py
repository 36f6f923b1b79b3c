#!/usr/bin/env python3
"""Time of unetdc_label_neighbors (csrc/neighbors.hip) on 1040 x 1388 label maps: the bright discs of
tools/quantify_e2e.py's synthetic micrographs labelled by unetdc_ccl_labels, an empty map and one label over the whole image,
next to its yardsticks (unetdc_ccl_labels + unetdc_label_props on the same mask, neighbor_pairs_numpy on the host).
    python3 tools/neighbors_bench.py [--calls N] [--windows W] [--once]
HIP events around N back-to-back calls, median (min .. max) of W windows.  --once: one call per case and no host yardstick
(for a kernel trace)."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from unet_dc_segmentation_amd import _lib
from utils import droplet_neighbors as dn

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


def main():
    once = "--once" in sys.argv
    calls, windows = (1, 1) if once else (arg("--calls", 50), arg("--windows", 5))
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    cap = 1 << 14
    mask = torch.from_numpy((bench.synthetic_micrograph(7)[..., 0] > 125).astype(np.uint8)).cuda()
    ws = torch.empty(max(lib.unetdc_ccl_labels_workspace(H, W), lib.unetdc_label_neighbors_workspace(H, W, cap, 1 << 14)),
                     dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    area = torch.empty(cap, dtype=torch.int32, device="cuda")
    sums = torch.empty(2 + 14, cap, dtype=torch.int64, device="cuda")
    label = torch.empty(H, W, dtype=torch.int32, device="cuda")
    pairs = torch.empty(3, 1 << 14, dtype=torch.int32, device="cuda")
    cols = torch.empty(5, cap, dtype=torch.int32, device="cuda")

    def label_it():
        _lib.call("unetdc_ccl_labels", mask.data_ptr(), H, W, 1, ws.data_ptr(), ws.numel(), count.data_ptr(), area.data_ptr(),
                  sums[0].data_ptr(), sums[1].data_ptr(), None, label.data_ptr(), cap, s)
        _lib.call("unetdc_label_props", label.data_ptr(), None, H, W, sums[2].data_ptr(), cap, s)

    def neighbors(lab, G):
        _lib.call("unetdc_label_neighbors", lab.data_ptr(), cap, H, W, G, ws.data_ptr(), ws.numel(), count[1:].data_ptr(),
                  *(pairs[j].data_ptr() for j in range(3)), pairs.shape[1], *(cols[j].data_ptr() for j in range(5)), s)

    label_it()
    lab_h = label.cpu().numpy()
    k = int(count[0].item())
    dx, dy, edge = lab_h[:, 1:] != lab_h[:, :-1], lab_h[1:] != lab_h[:-1], np.zeros(lab_h.shape, bool)
    edge[:, 1:] |= dx
    edge[:, :-1] |= dx
    edge[1:] |= dy
    edge[:-1] |= dy
    border = int((edge & (lab_h > 0)).sum())
    print(f"one MI355X; HIP events around {calls} back-to-back calls, median (min .. max) of {windows} windows, us per call")
    print(f"label map {H} x {W}: {k} droplets, foreground {float((lab_h > 0).mean()):.3f}, {border} border pixels")
    print(f"unetdc_ccl_labels + unetdc_label_props (yardstick)      : {timed(label_it, calls, windows)}")
    label_it()
    cases = [("synthetic droplets", label), ("empty", torch.zeros_like(label)), ("one label", torch.ones_like(label))]
    for G in (5, 20, 64):
        for name, lab in cases:
            t = timed(lambda: neighbors(lab, G), calls, windows)
            print(f"unetdc_label_neighbors G={G:2d} {name:18s}            : {t}; {int(count[1].item())} pairs")
    if once:
        return
    for G in (5, 20, 64):
        t0 = time.perf_counter()
        n = len(dn.neighbor_pairs_numpy(lab_h, k, G)[0])
        print(f"neighbor_pairs_numpy (host) G={G:2d} synthetic droplets      : {(time.perf_counter() - t0) * 1e3:9.1f} ms; {n} pairs")


if __name__ == "__main__":
    main()
