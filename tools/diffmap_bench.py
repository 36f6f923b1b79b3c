#!/usr/bin/env python3
"""Time of unetdc_diff_regions and unetdc_diff_paint (csrc/diffmap.hip) at 1040 x 1388, next to their
comparator: utils.difference_map.diff_regions_numpy + difference_map_rgb + overlay_difference on the same planes on this host.
    python3 tools/diffmap_bench.py [CASE ...] [--calls N] [--windows W]
CASE: moved (the annotation moved by one pixel: thin rims, the usual picture), dilated, unrelated (two independent masks),
micrograph (bench.synthetic_micrograph's discs against themselves moved by two pixels), black (nothing set: one region of
1.4 M pixels, every add of the stats pass on one root).  Default: all.  HIP events around N back-to-back calls, median (min ..
max) of W windows.  Under a kernel trace the per-kernel times are the ones to read: the merge against the stats pass."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import diffmap_ref as R
from unet_dc_segmentation_amd import _lib
from utils import difference_map as D

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


def planes(case):
    if case == "black":
        z = np.zeros((H, W), np.uint8)
        return z, z.copy()
    if case == "micrograph":
        import bench
        gt = (bench.synthetic_micrograph(7)[..., 0] > 125).astype(np.uint8)
        return R.shifted(gt, 2, 2), gt
    return R.realistic(H, W, case, seed=5)


def host_ms(fn, repeats=3):
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    cases = [a for a in sys.argv[1:] if not a.startswith("--") and not a.isdigit()] or ["moved", "dilated", "unrelated", "micrograph", "black"]
    calls, windows = arg("--calls", 20), arg("--windows", 5)
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    nbytes = lib.unetdc_diff_regions_workspace(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rgb_h = np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)
    rgb = torch.from_numpy(rgb_h).cuda()
    cap = H * W
    head = torch.zeros(13, dtype=torch.int64, device="cuda")
    i32 = torch.empty(3, cap, dtype=torch.int32, device="cuda")
    i64 = torch.empty(2, cap, dtype=torch.int64, device="cuda")
    diff, over = (torch.empty(H, W, 3, dtype=torch.uint8, device="cuda") for _ in range(2))
    for case in cases:
        pred_h, gt_h = planes(case)
        pred, gt = torch.from_numpy(pred_h).cuda(), torch.from_numpy(gt_h).cuda()

        def regions():
            _lib.call("unetdc_diff_regions", pred.data_ptr(), gt.data_ptr(), H, W, 1, ws.data_ptr(), nbytes, head.data_ptr(),
                      head[12:].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), i64[0].data_ptr(), i64[1].data_ptr(),
                      i32[2].data_ptr(), cap, s)

        def paint(both=True):
            _lib.call("unetdc_diff_paint", pred.data_ptr(), gt.data_ptr(), rgb.data_ptr(), H, W, diff.data_ptr(),
                      over.data_ptr() if both else None, s)

        regions()
        paint()
        want = D.diff_regions_numpy(pred_h, gt_h, 1)
        n = len(want["class"])
        assert np.array_equal(head[:12].cpu().numpy(), want["image"]) and int(head[12]) == n
        assert np.array_equal(i32[1, :n].cpu().numpy(), want["area"]) and np.array_equal(i64[1, :n].cpu().numpy(), want["sumx"])
        assert np.array_equal(over.cpu().numpy(), D.overlay_difference(rgb_h, pred_h, gt_h))
        im = want["image"]
        print(f"{case}: {H} x {W}, pixels {im[:4].tolist()}, regions {im[4:8].tolist()} (black, green, red, yellow), {n} table rows")
        print(f"  unetdc_diff_regions                     {timed(regions, calls, windows)}")
        print(f"  unetdc_diff_paint, both pictures        {timed(paint, calls, windows)}")
        print(f"  unetdc_diff_paint, the map alone        {timed(lambda: paint(False), calls, windows)}")
        print(f"  host: diff_regions_numpy                {host_ms(lambda: D.diff_regions_numpy(pred_h, gt_h, 1)):9.1f} ms (best of 3)")
        print(f"  host: difference_map_rgb + overlay      "
              f"{host_ms(lambda: (D.difference_map_rgb(pred_h, gt_h), D.overlay_difference(rgb_h, pred_h, gt_h))):9.1f} ms (best of 3)")


if __name__ == "__main__":
    main()
