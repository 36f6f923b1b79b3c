#!/usr/bin/env python3
"""Time of the polygon rasteriser (csrc/polyfill.hip, unet_dc_segmentation_amd/polygons.py) on one
1040 x 1388 frame of about 1 700 disc outlines, the annotation utils/droplet_outlines.py writes for a noise mask:
    python3 tools/polygons_bench.py [--calls N] [--windows W] [--discs D]
Device time per image of the three entry points from HIP events around N back-to-back calls, median (min .. max) of W windows,
and of rasterize_batch as a whole (host packing of the upload, the census wait and the relabel included) by the wall clock.
Next to it on the host: rasterize_numpy (the restatement), PIL.ImageDraw.polygon (a TIMING yardstick only: its inside rule is
another one) and the JSON parse + pack of the file, which no device helps with.  The device result is checked against
rasterize_numpy before anything is timed."""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageDraw

from unet_dc_segmentation_amd import _lib
from unet_dc_segmentation_amd.polygons import rasterize_batch
from utils import droplet_outlines as do
from utils import polygon_masks as pm

H, W = 1040, 1388


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def disc_labels(n, seed=28):
    """n discs of radius 4..14 on the frame, label k where disc k is drawn and nothing was before."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[-14:15, -14:15]
    for k in range(1, n + 1):
        r, cy, cx = int(rng.integers(4, 15)), int(rng.integers(15, H - 15)), int(rng.integers(15, W - 15))
        view = lab[cy - 14:cy + 15, cx - 14:cx + 15]
        view[(yy * yy + xx * xx <= r * r) & (view == 0)] = k
    return lab


def device_timed(fn, calls, windows):
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
    return f"{np.median(out):10.1f} us ({min(out):.1f} .. {max(out):.1f})"


def host_timed(fn, repeats=3):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return f"{np.median(out):10.1f} us ({min(out):.1f} .. {max(out):.1f})"


def main():
    calls, windows, discs = arg("--calls", 20), arg("--windows", 5), arg("--discs", 1700)
    lab = disc_labels(discs)
    text = json.dumps(do.geojson(do.outlines_numpy(lab), "frame"))
    feats = pm.features_of_geojson(json.loads(text))
    packed = pm.pack(feats)
    P, R, V = len(packed["poly_label"]), len(packed["ring_first"]) - 1, len(packed["verts"])
    want = pm.rasterize_numpy(packed, H, W, compact=True)
    assert np.array_equal(pm.rasterize_numpy(packed, H, W)["labels"], lab)                  # export -> import is the identity
    rec = rasterize_batch([packed], [(H, W)], compact=True)[0]
    assert np.array_equal(rec["labels"].cpu().numpy(), want["labels"]) and np.array_equal(rec["area"], want["area"])
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in packed.items()}
    out = torch.empty(H, W, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.unetdc_polygon_fill_workspace(H, W, P, R, V), dtype=torch.uint8, device="cuda")
    area = torch.empty(P, dtype=torch.int64, device="cuda")
    lut = torch.arange(1, P + 1, dtype=torch.int32, device="cuda")
    fill = lambda: _lib.call("unetdc_polygon_fill", d["verts"].data_ptr(), d["ring_first"].data_ptr(), d["poly_first_ring"].data_ptr(),      # noqa: E731
                             d["poly_label"].data_ptr(), P, R, V, H, W, out.data_ptr(), ws.data_ptr(), ws.numel(), s)
    census = lambda: _lib.call("unetdc_label_census", out.data_ptr(), H, W, P, area.data_ptr(), s)                                          # noqa: E731
    relabel = lambda: _lib.call("unetdc_label_relabel", out.data_ptr(), H, W, lut.data_ptr(), P, s)                                         # noqa: E731

    def pil():
        im = Image.new("I", (W, H), 0)
        draw = ImageDraw.Draw(im)
        for f in feats:
            for poly in f["polygons"]:
                draw.polygon([tuple(p) for p in poly[0].tolist()], fill=f["label"])
        return im

    print(f"{H} x {W}: {len(feats)} features, {P} polygons, {R} rings, {V} vertices, {len(text)} bytes of GeoJSON, "
          f"{int(np.count_nonzero(lab))} pixels inside")
    print(f"  unetdc_polygon_fill (clear, items, scan, fill)   {device_timed(fill, calls, windows)}")
    print(f"  unetdc_label_census                              {device_timed(census, calls, windows)}")
    print(f"  unetdc_label_relabel                             {device_timed(relabel, calls, windows)}")
    print(f"  rasterize_batch, one image, wall clock           {host_timed(lambda: (rasterize_batch([packed], [(H, W)]), torch.cuda.synchronize()), 9)}")
    print(f"  rasterize_numpy (host restatement)               {host_timed(lambda: pm.rasterize_numpy(packed, H, W, compact=True))}")
    print(f"  PIL.ImageDraw.polygon (timing yardstick only)    {host_timed(pil)}")
    print(f"  json.loads + features_of_geojson                 {host_timed(lambda: pm.features_of_geojson(json.loads(text)))}")
    print(f"  pack                                             {host_timed(lambda: pm.pack(feats))}")


if __name__ == "__main__":
    main()
