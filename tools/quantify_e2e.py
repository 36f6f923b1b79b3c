#!/usr/bin/env python3
"""End-to-end throughput of the quantify_droplets_batch.py SCRIPT (file decode, preprocessing, network, droplet tables,
mask PNG + CSV writes) on N synthetic 1040 x 1388 micrographs written as PNG files:
    python3 tools/quantify_e2e.py [N] [dtype] [--density_maps] [--split_touching] [--droplet_shape] [--gt]
                                  [--prob_thresh_low T] [--fill_holes[=N]] [--thresh_sweep[=K]] [--sweep_objects=T,T...]
                                  [--tile[=T]] [--tile_overlap=O] [--batch=B] [--tta[=N]] [--neighbors[=G]]
                                  [--boundary[=R]] [--boundary_tol=T,T...] [--confidence[=BAND]] [--confidence_maps]
                                  [--droplet_hull[=S]] [--diff_maps[=MIN_AREA]] [--spatial_stats[=R]] [--spatial_sims=S]
                                  [--outlines] [--deep] [--intensity_window[=PLO,PHI]] [--intensity_levels=LO,HI]
                                  [--nuclei[=N]] [--cell_radius=R]
--density_maps: the density arm (ROI, radial and spatial maps on the device, two heat-map PNGs per image).
--split_touching: the split arm (distance transform, basins and merging on the device, one label PNG per image; default depth).
--droplet_shape: the shape arm (label map, per-droplet shape and intensity integers on the device, the extra CSV columns).
--gt: the matching arm (--gt_dir: annotated masks labelled and the overlap table built on the device, gt_droplets.csv and
match_per_image.csv); the annotation of a synthetic micrograph is its own bright discs, cut out by a grey threshold.
--prob_thresh_low T, --fill_holes or --fill_holes=N: passed through to the script (the mask-cleaning arm: hysteresis and hole
filling on the device).
--thresh_sweep or --thresh_sweep=K, --sweep_objects=T,T...: passed through to the script (the threshold-sweep arm: the pixel
confusion matrix at every threshold of the grid on the device, threshold_sweep.csv); they switch --gt on.
--tile or --tile=T, --tile_overlap=O, --batch=B: passed through to the script (the tile arm: the network runs on overlapping
tiles of the native-size image, B per forward, blended on the device; the checkpoint is the same seeded one in both arms).
--tta or --tta=N: passed through to the script (the test-time-augmentation arm: N variants of every input or tile through the
network, mapped back and averaged on the device).
--neighbors or --neighbors=G: passed through to the script (the neighbourhood arm: contact pairs, nearest contact, degree and
cluster per droplet on the device, the extra CSV columns and droplet_contacts.csv).
--boundary or --boundary=R, --boundary_tol=T,T...: passed through to the script, implies --gt (the boundary arm: surface distances
between predicted and annotated label maps on the device, the extra CSV columns and boundary_per_image.csv).
--confidence or --confidence=BAND, --confidence_maps: passed through to the script (the confidence arm: per-droplet probability,
entropy and, with --tta, variant-disagreement integers on the device, the extra CSV columns and confidence_per_image.csv).
--droplet_hull or --droplet_hull=S: passed through to the script (the hull arm: per-droplet convex hull, solidity and Feret
integers on the device, the extra CSV columns).
--diff_maps or --diff_maps=MIN_AREA: passed through to the script, implies --gt (the difference-map arm: 8-connected regions of the
class plane and both pictures on the device, two more PNGs per image, diff_regions.csv and diff_regions_per_image.csv).
--spatial_stats or --spatial_stats=R, --spatial_sims=S, --spatial_seed=N: passed through to the script (the spatial-statistics arm:
Ripley counts of the droplet centroids and of the simulated patterns on the device, spatial_stats.csv and spatial_per_image.csv).
--outlines: passed through to the script (the outline arm: crack-following contours of the label map on the device, the extra CSV
columns, one GeoJSON file per image and outlines_coco.json).
--gt_polygons: the matching arm on polygon annotations (--gt_polygons DIR: the discs' outlines as one GeoJSON file per image,
filled on the device); --gt_labels: its yardstick, the same annotations as the 16-bit label images those polygons fill to
(--gt_dir DIR --gt_labels).  Both imply --gt.
--deep: the files are 16-bit grey PNGs (the micrograph's grey x 16 plus four bits of noise, a 12-bit camera's range);
--intensity_window or --intensity_window=PLO,PHI, --intensity_levels=LO,HI: passed through to the script (the window arm: ranks
and the window to 8 bits on the device, intensity_per_image.csv).  --deep without a window flag is the clipped decode.
--nuclei or --nuclei=N, --cell_radius=R: the droplets-per-cell arm (--nuclei_dir: N seeded discs per image, default 50, as binary
masks; their territories and the per-cell table on the device, the extra CSV columns, cells.csv, cells_per_image.csv and one
16-bit territory PNG per image)."""
import os
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

import bench
import quantify_droplets_batch as qdb
from models.model_2 import UNetDC

density = "--density_maps" in sys.argv
split = "--split_touching" in sys.argv
shape = "--droplet_shape" in sys.argv
gt = "--gt" in sys.argv
clean_argv = []
if "--prob_thresh_low" in sys.argv:                       # the one flag here that takes a separate value
    k = sys.argv.index("--prob_thresh_low")
    clean_argv += sys.argv[k:k + 2]
    del sys.argv[k:k + 2]
clean_argv += [a for a in sys.argv[1:] if a.split("=")[0] == "--fill_holes"]
sweep_argv = [a for a in sys.argv[1:] if a.split("=")[0] in ("--thresh_sweep", "--sweep_objects")]
gt = gt or bool(sweep_argv)
tile_argv = [a for a in sys.argv[1:] if a.split("=")[0] in ("--tile", "--tile_overlap", "--batch")]
tta_argv = [a for a in sys.argv[1:] if a.split("=")[0] == "--tta"]
nb_argv = [a for a in sys.argv[1:] if a.split("=")[0] == "--neighbors"]
bd_argv = [a for a in sys.argv[1:] if a.split("=")[0] in ("--boundary", "--boundary_tol")]
gt = gt or bool(bd_argv)
cf_argv = [a for a in sys.argv[1:] if a.split("=")[0] in ("--confidence", "--confidence_maps")]
hl_argv = [a for a in sys.argv[1:] if a.split("=")[0] == "--droplet_hull"]
df_argv = [a for a in sys.argv[1:] if a.split("=")[0] == "--diff_maps"]
gt = gt or bool(df_argv)
sp_argv = [a for a in sys.argv[1:] if a.split("=")[0] in ("--spatial_stats", "--spatial_sims", "--spatial_seed")]
ol_argv = [a for a in sys.argv[1:] if a == "--outlines"]
iw_argv = [a for a in sys.argv[1:] if a.split("=")[0] in ("--intensity_window", "--intensity_levels")]
nuc_argv = [a for a in sys.argv[1:] if a.split("=")[0] == "--nuclei"]
cell_argv = [a.replace("=", " ").split() for a in sys.argv[1:] if a.split("=")[0] == "--cell_radius"]
deep = "--deep" in sys.argv
gt_polygons, gt_label_files = "--gt_polygons" in sys.argv, "--gt_labels" in sys.argv
gt = gt or gt_polygons or gt_label_files
pos = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(pos[0]) if len(pos) > 0 else 64
dtype = pos[1] if len(pos) > 1 else "bf16"
with tempfile.TemporaryDirectory() as d:
    ind, out = os.path.join(d, "in"), os.path.join(d, "out")
    os.makedirs(ind)
    imgs = [bench.synthetic_micrograph(7 + i % 8) for i in range(n)]
    for i, im in enumerate(imgs):
        if deep:
            g = im[..., 0].astype(np.uint16) * 16 + np.random.default_rng(i).integers(0, 16, im.shape[:2]).astype(np.uint16)
            Image.fromarray(g).save(os.path.join(ind, f"img_{i:04d}.png"))
        else:
            Image.fromarray(im).save(os.path.join(ind, f"img_{i:04d}.png"))
    gt_argv = []
    if gt and (gt_polygons or gt_label_files):            # the same discs as polygons, or as the label images they fill to
        import json
        from utils import droplet_outlines as do
        from utils import polygon_masks as pm
        from utils.droplet_match import gt_labels_numpy
        gtd = os.path.join(d, "gt")
        os.makedirs(gtd)
        docs = {}
        for i, im in enumerate(imgs):
            if 7 + i % 8 not in docs:
                lab = gt_labels_numpy(im[..., 0] > 125, 4)
                doc = do.geojson(do.outlines_numpy(lab), "gt")
                docs[7 + i % 8] = (json.dumps(doc), pm.rasterize_numpy(pm.pack(pm.features_of_geojson(doc)), *lab.shape, compact=True)["labels"])
            text, filled = docs[7 + i % 8]
            if gt_polygons:
                with open(os.path.join(gtd, f"img_{i:04d}.geojson"), "w") as fh:
                    fh.write(text)
            else:
                Image.fromarray(filled.astype(np.uint16)).save(os.path.join(gtd, f"img_{i:04d}.png"))
        gt_argv = ["--gt_polygons", gtd] if gt_polygons else ["--gt_dir", gtd, "--gt_labels"]
    elif gt:                                              # the discs are 90 grey levels above a background of 40..90
        gtd = os.path.join(d, "gt")
        os.makedirs(gtd)
        for i, im in enumerate(imgs):
            Image.fromarray((im[..., 0] > 125).astype(np.uint8) * 255).save(os.path.join(gtd, f"img_{i:04d}.png"))
        gt_argv = ["--gt_dir", gtd, "--gt_min_area", "4"]
    if nuc_argv:                                          # seeded discs of radius 12, one binary mask per image
        from tools.cells_bench import nuclei
        nd = os.path.join(d, "nuclei")
        os.makedirs(nd)
        n_nuclei = int(nuc_argv[0].split("=")[1]) if "=" in nuc_argv[0] else 50
        masks = [Image.fromarray((nuclei(n_nuclei, seed) > 0).astype(np.uint8) * 255) for seed in range(8)]
        for i in range(n):
            masks[i % 8].save(os.path.join(nd, f"img_{i:04d}.png"))
        gt_argv += ["--nuclei_dir", nd] + [v for a in cell_argv for v in a]
    torch.manual_seed(0)
    m = UNetDC(in_channels=3, out_channels=1)
    if torch.cuda.is_available():                         # calibrate the head bias so that ~10 % of the pixels are "droplet"
        from unet_dc_segmentation_amd.preprocess import preprocess_device
        md = m.cuda().eval()
        md.set_compute_dtype(dtype)
        with torch.no_grad():
            p0 = md(torch.stack([preprocess_device(im, 50, 512, "cuda") for im in imgs[:8]])).clamp(1e-6, 1 - 1e-6)
            z = torch.log(p0 / (1 - p0)).flatten()[::7]
            md.out_conv.bias += float(np.log(0.3 / 0.7)) - float(torch.quantile(z, 0.9))
        m = md
    ck = os.path.join(d, "ck.pth")
    torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()}, ck)
    argv = ["--img_dir", ind, "--ckpt_path", ck, "--out_dir", out, "--dtype", dtype, "--skip_excel", "--skip_histogram"]
    argv += ["--density_maps"] if density else []
    argv += ["--split_touching"] if split else []
    argv += ["--droplet_shape"] if shape else []
    argv += gt_argv + clean_argv + sweep_argv + tile_argv + tta_argv + nb_argv + bd_argv + cf_argv + hl_argv + df_argv + sp_argv + ol_argv + iw_argv
    qdb.main(argv)                                        # warm-up (library load, engine construction)
    t0 = time.perf_counter()
    qdb.main(argv)
    dt = time.perf_counter() - t0
    print(f"quantify_droplets_batch.py end to end: {n} files in {dt:.2f} s = {n / dt:.1f} images/s ({dtype}, device {qdb.DEVICE}{', density maps' if density else ''}{', split touching' if split else ''}{', droplet shape' if shape else ''}{', gt matching' if gt else ''}{' --gt_polygons' if gt_polygons else ' --gt_labels' if gt_label_files else ''}{', mask cleaning' if clean_argv else ''}{', threshold sweep' if sweep_argv else ''}{', tiled ' + ' '.join(tile_argv) if tile_argv else ''}{', ' + tta_argv[0] if tta_argv else ''}{', ' + nb_argv[0] if nb_argv else ''}{', ' + bd_argv[0] if bd_argv else ''}{', ' + ' '.join(cf_argv) if cf_argv else ''}{', ' + hl_argv[0] if hl_argv else ''}{', ' + df_argv[0] if df_argv else ''}{', ' + ' '.join(sp_argv) if sp_argv else ''}{', --outlines' if ol_argv else ''}{', 16-bit files' if deep else ''}{', ' + ' '.join(iw_argv) if iw_argv else ''}{', ' + ' '.join(nuc_argv + [' '.join(a) for a in cell_argv]) if nuc_argv else ''})")
