#!/usr/bin/env python3
"""Time of unetdc_label_nearest and unetdc_cell_table (csrc/cells.hip) at 1040 x 1388: nuclei are discs of
radius 12 at seeded random centres, 50 and 500 of them, the territories unbounded and cut at R = 150; the droplet map is the
bright discs of tools/quantify_e2e.py's synthetic micrographs labelled by unetdc_ccl_labels.
    python3 tools/cells_bench.py [--calls N] [--windows W] [--once]
HIP events around N back-to-back calls, median (min .. max) of W windows.  --once: every case once, for a kernel trace, which
is where the column pass and the row pass of unetdc_label_nearest are told apart.
Bytes/s is against the algorithmic bytes of unetdc_label_nearest: the label map in, two planes out (12 bytes per pixel)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from unet_dc_segmentation_amd import _lib
from unet_dc_segmentation_amd.droplets import TRIPLE_ROOM

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


def nuclei(n, seed=0, r=12):
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disc = yy * yy + xx * xx <= r * r
    for k in range(n):
        cy, cx = int(rng.integers(r, H - r)), int(rng.integers(r, W - r))
        view = lab[cy - r:cy + r + 1, cx - r:cx + r + 1]
        view[disc & (view == 0)] = k + 1
    return lab


def main():
    once = "--once" in sys.argv
    calls, windows = (1, 1) if once else (arg("--calls", 20), arg("--windows", 5))
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    cap = 1 << 14
    room = min(TRIPLE_ROOM, H * W)                           # what droplets.py gives the first launch
    gray = bench.synthetic_micrograph(7)[..., 0]
    mask = torch.from_numpy((gray > 125).astype(np.uint8)).cuda()
    ws = torch.empty(max(lib.unetdc_ccl_labels_workspace(H, W), lib.unetdc_label_nearest_workspace(H, W),
                         lib.unetdc_cell_table_workspace(H, W, cap, 0, room)), dtype=torch.uint8, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    area = torch.empty(cap, dtype=torch.int32, device="cuda")
    sums = torch.empty(2, cap, dtype=torch.int64, device="cuda")
    drop = torch.empty(H, W, dtype=torch.int32, device="cuda")
    _lib.call("unetdc_ccl_labels", mask.data_ptr(), H, W, 1, ws.data_ptr(), ws.numel(), count.data_ptr(), area.data_ptr(),
              sums[0].data_ptr(), sums[1].data_ptr(), None, drop.data_ptr(), cap, s)
    k = int(count[0].item())
    terr, d2 = torch.empty_like(drop), torch.empty_like(drop)
    per_droplet = torch.empty(6, cap, dtype=torch.int32, device="cuda")
    print(f"one MI355X; HIP events around {calls} back-to-back calls, median (min .. max) of {windows} windows, us per call")
    print(f"maps {H} x {W}; droplet map: {k} droplets, foreground {float(mask.float().mean()):.3f}; droplet capacity {cap}, pair room {room}")
    for n in (50, 500):
        nuc = torch.from_numpy(nuclei(n)).cuda()
        per_cell = torch.empty(8, n, dtype=torch.int64, device="cuda")
        for radius in (0, 150):
            def nearest():
                _lib.call("unetdc_label_nearest", nuc.data_ptr(), n, H, W, radius, ws.data_ptr(), ws.numel(), terr.data_ptr(), d2.data_ptr(), s)

            def table():
                _lib.call("unetdc_cell_table", drop.data_ptr(), cap, terr.data_ptr(), n, d2.data_ptr(), H, W, ws.data_ptr(), ws.numel(),
                          count[1:].data_ptr(), room, per_droplet.data_ptr(), per_cell.data_ptr(), s)
            t, text = timed(nearest, calls, windows)
            far = int(d2.max().item()) ** 0.5
            print(f"unetdc_label_nearest {n:3d} nuclei, R = {radius:3d}: {text}  = {12 * H * W / t / 1e3:7.1f} GB/s of the algorithmic bytes"
                  f"   (farthest pixel {far:.0f} px, {int((terr == 0).sum().item())} pixels in no cell)")
            t, text = timed(table, calls, windows)
            print(f"unetdc_cell_table    {n:3d} cells,  R = {radius:3d}: {text}   ((droplet, cell) pairs {int(count[1].item())})")


if __name__ == "__main__":
    main()
