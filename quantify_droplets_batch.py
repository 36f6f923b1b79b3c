#!/usr/bin/env python3
"""Batch inference + droplet quantification -- drop-in for the reference's
``quantify_droplets_batch.py`` (same CLI flags: the Tk/Qt front-ends build this argv,
gui.py:26-39, gui_qt.py:372-400; same output files and CSV columns, outputs/all_droplets.csv:1).

Flow (reference lines): load_model :34-37 -> preprocess :40-46 (RGB, rolling ball, resize 512, /255)
-> run_batch :48-79 (model(batch) under no_grad, ``> thresh`` on the probabilities, nearest resize
to the original size, mask PNG, per-image CSV) -> quantify :81-95 (4-connected components, area
filter, area / equivalent diameter / centroid) -> summary CSV / XLSX / histogram :163-199.
The network runs on the HIP kernels when a GPU is present (``DEVICE = "cuda"``), otherwise on
PyTorch-CPU exactly like the reference.  On the GPU the threshold, the nearest-neighbour resize to the original
size, the connected-component labelling and the per-droplet sums run on the device as well
(unet_dc_segmentation_amd/droplets.py, csrc/ccl.hip): only the uint8 mask and three integers per droplet are
copied back.  cv2 / scikit-image are optional on the CPU path: SciPy's ``ndimage.label`` with its default
cross-shaped structure is skimage's ``label(connectivity=1)``; the resize of the mask to the original size reproduces what the
reference's call computes (its interpolation flag sits in the positional slot of ``dst``, so OpenCV's default 8-bit bilinear
runs on the {0,1} mask: unet_dc_segmentation_amd/droplets.py:MASK_RESIZE).
``--split_touching`` counts a droplet per basin of the mask's distance transform instead of per connected component
("Splitting touching droplets": csrc/split.hip on the device, utils/droplet_split.py on the CPU) and writes a
16-bit label image next to every mask.
``--droplet_shape`` adds the shape and intensity columns of DESIGN.md section 11 to every droplet table (perimeter,
circularity, axes, eccentricity, orientation, bounding box, touches_border, intensity of the original image): exact integers
per droplet from csrc/shape.hip on the device or utils/droplet_shape.py on the CPU, one derivation for both.
``--gt_dir D`` scores every image against its annotated mask D/NAME.* (DESIGN.md section 12): the overlap table of the
predicted and the annotated label map from csrc/match.hip on the device or utils/droplet_match.py on the CPU, one derivation
for both; adds gt_label / gt_iou / gt_covered to the droplet tables and writes gt_droplets.csv and match_per_image.csv.
``--prob_thresh_low T`` / ``--fill_holes [N]`` clean the mask before anything reads it: hysteresis
thresholding between T and --prob_thresh, then holes of at most N pixels (any size without N) are filled; csrc/clean.hip on the
device, utils/droplet_clean.py on the CPU.  The cleaned mask is the one every output sees; mask_clean_per_image.csv says
what was changed per image.
``--thresh_sweep [K]`` (with ``--gt_dir``) scores the raw thresholded mask against the annotation, pixel by pixel, at the K
thresholds k / K in one pass per image (csrc/sweep.hip on the device, utils/threshold_sweep.py on the
CPU) and writes threshold_sweep.csv pooled over all images; ``--sweep_objects T[,T...]`` repeats the droplet stage and the
matching of ``--gt_dir`` at the listed thresholds on the probabilities already computed and writes
threshold_sweep_objects.csv.
``--tile [T]`` / ``--tile_overlap O`` run the network at the image's NATIVE resolution instead of on the 512 x 512 squash
(DESIGN.md section 15): the rolling-ball-corrected image is cut into overlapping T x T tiles (512 without T, overlap 64), the tiles
go through the network ``--batch`` at a time, and their probabilities are blended into one map of the image's size
(csrc/tile.hip and unet_dc_segmentation_amd/tiling.py on the device, utils/tiling.py on the CPU, one derivation for both);
every option above then works on that map.  Meant for checkpoints trained at the scale they are applied at.
``--tta [N]`` averages the network over N flipped and rotated variants of every input (N in 1, 2, 4, 8; 8
without N): the variants go through the network ``--batch`` items at a time, every output is mapped back and the mean is the
probability map that every option above reads (csrc/tta.hip and unet_dc_segmentation_amd/tta.py on the device, utils/tta.py on
the CPU, one derivation for both); with ``--tile`` the variants are those of every tile.
"""
import argparse
from pathlib import Path

import numpy as np
import pandas as pd
import torch
from PIL import Image

from models.model_2 import UNetDC
from unet_dc_segmentation_amd.droplets import resize_mask_like_reference
from utils.data_loader import resize_image, rolling_ball_correction_rgb

DEVICE = "cuda" if torch.cuda.is_available() else "cpu"
IMG_SIZE = 512          # matches the training resize


def load_model(ckpt, dtype="f32"):
    m = UNetDC(in_channels=3, out_channels=1)
    m.load_state_dict(torch.load(ckpt, map_location=DEVICE, weights_only=True))
    m.set_compute_dtype(dtype)
    return m.to(DEVICE).eval()


def decode_rgb(path):
    """File -> uint8 RGB array (runs in the decode pool: PIL releases the GIL while it inflates)."""
    return np.array(Image.open(path).convert("RGB"))


def preprocess(path, background_radius, im=None, keep_rgb=False):
    """-> (network input, (oh, ow)), and with keep_rgb the decoded original image as well (a device tensor on the GPU
    path: the density maps read it there without a second upload)."""
    im = decode_rgb(path) if im is None else im
    oh, ow = im.shape[:2]
    if DEVICE == "cuda":                                 # rolling ball + resize + /255 + CHW on the GPU (csrc/preprocess.hip)
        from unet_dc_segmentation_amd.preprocess import preprocess_device
        if keep_rgb:
            x, rgb = preprocess_device(im, background_radius, IMG_SIZE, DEVICE, return_rgb=True)
            return x, (oh, ow), rgb
        return preprocess_device(im, background_radius, IMG_SIZE, DEVICE), (oh, ow)
    if keep_rgb:
        t, osize = preprocess(path, background_radius, im)
        return t, osize, im
    im = rolling_ball_correction_rgb(im, background_radius)
    im = resize_image(im, IMG_SIZE).astype(np.float32) / 255.0
    return torch.from_numpy(im).permute(2, 0, 1), (oh, ow)


def predict_tiled_image(model, im, background_radius, tile, batch, keep_rgb=False, tta=None):
    """--tile: decoded image -> (probabilities [1, 1, H, W] at the image's own size, the original image for the density maps or
    None).  Preprocessing is the rolling ball alone, at native size; then the tiles, `batch` per forward, and the blend.
    tta: the options of --tta, every tile's probabilities are then the mean over its variants."""
    more = {} if tta is None else {"tta": tta["N"]}
    if DEVICE == "cuda":
        from unet_dc_segmentation_amd.preprocess import MAX_ELEMENT, _upload, rolling_ball_device
        from unet_dc_segmentation_amd.tiling import predict_tiled
        host_ball = int(background_radius) > MAX_ELEMENT     # the element does not fit the kernel's LDS tile: host operator
        rgb = _upload(im, DEVICE) if keep_rgb or not host_ball else None
        corrected = (_upload(rolling_ball_correction_rgb(im, int(background_radius)), DEVICE) if host_ball
                     else rolling_ball_device(rgb, background_radius))
        return predict_tiled(model, corrected, tile["T"], tile["O"], batch, **more)[None, None], rgb
    from utils.tiling import predict_tiled_cpu
    p = predict_tiled_cpu(model, rolling_ball_correction_rgb(im, background_radius), tile["T"], tile["O"], batch, **more)
    return torch.from_numpy(p)[None, None], (im if keep_rgb else None)


def _droplet_table(area, cen_row, cen_col, px_per_um):
    """DataFrame with the reference's columns (outputs/all_droplets.csv:1) from per-droplet areas and centroids given in
    label order; equivalent_diameter = sqrt(4 area / pi) (known answer: area 18224 -> 152.327, outputs/all_droplets.csv:2)."""
    n = len(area)
    if n == 0:
        return pd.DataFrame()
    area = np.asarray(area, dtype=np.int64)
    df = pd.DataFrame({"label": np.arange(1, n + 1), "area": area, "equivalent_diameter": np.sqrt(4.0 * area / np.pi),
                       "centroid-0": np.asarray(cen_row, dtype=np.float64), "centroid-1": np.asarray(cen_col, dtype=np.float64)})
    if px_per_um is not None:
        df["area_sqmicron"] = df["area"] / (px_per_um ** 2)
        df["eq_diam_micron"] = df["equivalent_diameter"] / px_per_um
    return df


def quantify_split(bin_mask, min_area, px_per_um, split_depth):
    """CPU path of --split_touching: (the per-droplet table of the split droplets, their int32 label map)."""
    from utils.droplet_split import half_pixels, split_labels
    labels, area, sy, sx, _ = split_labels(bin_mask, half_pixels(split_depth), min_area)
    d = np.maximum(area, 1)
    return _droplet_table(area, sy.astype(np.float64) / d, sx.astype(np.float64) / d, px_per_um), labels


def add_shape_columns(df, props, hw, px_per_um):
    """--droplet_shape: the columns of utils.droplet_shape.shape_columns behind the table's own."""
    if df.empty:
        return df
    from utils.droplet_shape import shape_columns
    for name, col in shape_columns(props, hw, px_per_um).items():
        df[name] = col
    return df


def quantify_shape(bin_mask, min_area, px_per_um, split_depth, gray):
    """CPU path of --droplet_shape: (table with the shape columns, label map or None without a split depth).  Centroids are
    the integer sums over the area, as on the device."""
    from scipy import ndimage
    from utils.droplet_shape import label_props_numpy
    if split_depth is not None:
        from utils.droplet_split import half_pixels, split_labels
        labels = split_labels(bin_mask, half_pixels(split_depth), min_area)[0]
    else:
        labels, n = ndimage.label(bin_mask)
        if n:
            keep = np.bincount(labels.ravel(), minlength=n + 1) >= max(min_area, 1)
            keep[0] = False
            labels = ndimage.label(keep[labels])[0]
    props = label_props_numpy(labels, gray)
    d = np.maximum(props["area"], 1)
    df = _droplet_table(props["area"], props["Sy"].astype(np.float64) / d, props["Sx"].astype(np.float64) / d, px_per_um)
    return add_shape_columns(df, props, bin_mask.shape, px_per_um), (labels if split_depth is not None else None)


IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".tif", ".tiff")


def find_gt_files(images, gt_dir):
    """--gt_dir: {image path: annotation path}, checked before anything runs.  The annotation of NAME.ext is
    gt_dir/NAME.<any image suffix>; a missing one, or one whose size differs from its image, ends the run (PIL reads the
    sizes from the headers, nothing is decoded)."""
    found = {}
    for img in images:
        cands = [q for q in sorted(Path(gt_dir).glob(img.stem + ".*")) if q.suffix.lower() in IMAGE_SUFFIXES and q.stem == img.stem]
        if not cands:
            raise SystemExit(f"--gt_dir: no annotated mask for {img.name} ({Path(gt_dir) / (img.stem + '.*')})")
        with Image.open(img) as a, Image.open(cands[0]) as b:
            if a.size != b.size:
                raise SystemExit(f"--gt_dir: {cands[0]} is {b.size[0]} x {b.size[1]}, its image {img.name} {a.size[0]} x {a.size[1]}")
        found[str(img)] = cands[0]
    return found


def decode_gt(path, as_labels):
    """Annotation file -> uint8 {0, 1} mask (convert("L") > 0, as SegmentationDataset reads it) or, with --gt_labels, the
    int32 label image as it is."""
    im = Image.open(path)
    if not as_labels:
        return (np.array(im.convert("L")) > 0).astype(np.uint8)
    return np.array(im if im.mode in ("1", "L", "P", "I", "I;16", "I;16B") else im.convert("I")).astype(np.int32)


def pred_labels_cpu(bin_mask, min_area, split_depth):
    """CPU path of --gt_dir: the int32 label map whose numbers are the rows of the droplet table."""
    if split_depth is not None:
        from utils.droplet_split import half_pixels, split_labels
        return split_labels(bin_mask, half_pixels(split_depth), min_area)[0]
    from utils.droplet_match import gt_labels_numpy
    return gt_labels_numpy(bin_mask, min_area)


def match_cpu(labels, area, gt_item, gt_min_area, gt_are_labels):
    """CPU path of --gt_dir for one image: what unet_dc_segmentation_amd.evaluate.match_batch returns per image."""
    from utils import droplet_match as dm
    glab = gt_item if gt_are_labels else dm.gt_labels_numpy(gt_item, gt_min_area)
    garea, gsy, gsx = dm.label_sums(glab)
    a, b, n = dm.overlap_table_numpy(labels, glab, len(area), len(garea))
    return {"a": a, "b": b, "n": n, "gt_area": garea, "gt_sumy": gsy, "gt_sumx": gsx,
            "columns": dm.match_columns(area, garea, a, b, n)}


def add_match_outputs(gt, df, res, filename):
    """--gt_dir: the three columns behind the droplet table's own, this image's rows of gt_droplets.csv and its integers."""
    from utils.droplet_match import gt_table
    if not df.empty:
        for name, col in res["columns"]["pred"].items():
            df[name] = col
    gt["tables"].append(pd.DataFrame(gt_table(filename, res["gt_area"], res["gt_sumy"], res["gt_sumx"], res["columns"]["gt"])))
    gt["images"].append((filename, res["columns"]["image"]))
    return df


def quantify(bin_mask, min_area, px_per_um, split_depth=None):
    """Per-droplet table: label, area, equivalent_diameter, centroid-0/1 (+ micron columns) -- CPU path (SciPy).
    split_depth (pixels): the table of the split droplets instead (utils/droplet_split.py)."""
    if split_depth is not None:
        return quantify_split(bin_mask, min_area, px_per_um, split_depth)[0]
    from scipy import ndimage
    lbl, n = ndimage.label(bin_mask)                     # 4-connectivity, labels in raster order of the first pixel
    if n:
        areas = np.bincount(lbl.ravel(), minlength=n + 1)
        keep = areas >= min_area
        keep[0] = False
        lbl, n = ndimage.label(keep[lbl])
    if n == 0:
        return pd.DataFrame()
    idx = np.arange(1, n + 1)
    area = np.bincount(lbl.ravel(), minlength=n + 1)[1:]
    cen = np.array(ndimage.center_of_mass(np.ones_like(lbl), lbl, idx)).reshape(n, 2)
    return _droplet_table(area, cen[:, 0], cen[:, 1], px_per_um)


def quantify_device(probs2d, thresh, out_hw, min_area, px_per_um):
    """The same table from the probability map still on the HIP device; also returns the uint8 mask (host) for the PNG."""
    from unet_dc_segmentation_amd.droplets import mask_and_droplets
    mask, area, cy, cx = mask_and_droplets(probs2d, thresh, out_hw, min_area)
    return mask.cpu().numpy(), _droplet_table(area, cy, cx, px_per_um)


def _outline(mask):
    from scipy import ndimage
    return mask.astype(bool) & ~ndimage.binary_erosion(mask.astype(bool), iterations=2)


def _write_outputs(mask, df, fpath, name, mask_dir, overlay_dir, labels=None):
    """The per-image files of run_batch (reference :66-79): mask PNG, droplet CSV, optional overlay; with --split_touching
    (labels given) the 16-bit label image as well, and the overlay's outline follows the cuts."""
    Image.fromarray(mask * 255).save(str(mask_dir / f"{name}_pred.png"))
    df.to_csv(mask_dir.parent / f"{name}_droplets.csv", index=False)
    if labels is not None:
        from utils.droplet_split import labels_u16
        Image.fromarray(labels_u16(labels)).save(str(mask_dir / f"{name}_labels.png"))
    if overlay_dir is not None:
        img = np.array(Image.open(fpath).convert("RGB"))
        img[_outline(mask)] = (0, 255, 0)
        if labels is not None:
            from utils.droplet_split import label_boundaries
            img[label_boundaries(labels)] = (0, 255, 0)
        Image.fromarray(img).save(str(overlay_dir / f"{name}_overlay.png"))


def _density(density, dres, rgb, mask, fpath, name, writers):
    """--density_maps for one image: the row of density_per_image.csv, and the two heat-map PNGs (colormap gather and deflate
    in the writer pool).  dres: the device results of the batch for this image, or None on the CPU path."""
    from utils import density as hd
    r = hd.density_maps(rgb, mask, density["nb_layers"], density["kernel"]) if dres is None else dres
    density["rows"].append(hd.csv_row(Path(fpath).name, r, density["nb_layers"]))
    job = (hd.write_pngs, r["radial_index"], r["spatial_index"], density["out_dir"], name)
    if writers is None:
        job[0](*job[1:])
    else:
        writers[1].append(writers[0].submit(*job))


def _cpu_mask(p2, thresh, ow, oh, clean):
    """CPU path: probabilities [h, w] (numpy fp32) -> the mask every stage sees at one threshold (resize, then the cleaning
    options of the run)."""
    mask = resize_mask_like_reference((p2 > np.float32(thresh)).astype(np.uint8), ow, oh)
    if clean is not None:
        from utils.droplet_clean import clean_mask
        weak = None
        if clean["low"] is not None:
            weak = resize_mask_like_reference((p2 > np.float32(clean["low"])).astype(np.uint8), ow, oh)
        mask = clean_mask(mask, weak, clean["holes"])[0]
    return mask


def sweep_step(sweep, probs, meta, gt, min_area, split_depth, clean):
    """--thresh_sweep for one batch: the batch's probabilities against its annotations at every threshold of the grid, added
    into the run's histogram (on the device: unetdc_thresh_sweep, nothing waits; on the CPU: sweep_hist_numpy).  Then, for
    every threshold of --sweep_objects, the droplet stage with the run's own split / clean options and the matching of
    --gt_dir once more on the same probabilities: the integers of one match_per_image.csv row per image and threshold."""
    hws = [m[1] for m in meta]
    if probs.is_cuda:
        from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
        from unet_dc_segmentation_amd.evaluate import match_batch, sweep_batch
        sweep["hist"] = sweep_batch(probs[:, 0], gt["items"], hws, sweep["K"], hist=sweep["hist"])
        opts = {"shape": True, "return_labels": True} if split_depth is None else {"split_depth": split_depth, "return_labels": True}
        if clean is not None:
            opts.update(thresh_low=clean["low"], max_hole_area=clean["holes"])
        for t in sweep["objects"]:
            out = mask_and_droplets_batch(probs[:, 0], t, hws, min_area, **opts)
            res = match_batch([o[4] for o in out], [o[1] for o in out], gt["items"], gt["min_area"], gt["labels"])
            sweep["object_images"][t].extend(r["columns"]["image"] for r in res)
        return
    from utils.droplet_match import label_sums
    from utils.threshold_sweep import sweep_hist_numpy
    p = probs[:, 0].numpy()
    for i, (oh, ow) in enumerate(hws):
        h = sweep_hist_numpy(p[i], gt["items"][i], (oh, ow), sweep["K"])
        sweep["hist"] = h if sweep["hist"] is None else sweep["hist"] + h
        for t in sweep["objects"]:
            plab = pred_labels_cpu(_cpu_mask(p[i], t, ow, oh, clean), min_area, split_depth)
            res = match_cpu(plab, label_sums(plab)[0], gt["items"][i], gt["min_area"], gt["labels"])
            sweep["object_images"][t].append(res["columns"]["image"])


@torch.no_grad()
def run_batch(tensors, meta, model, mask_dir, overlay_dir, thresh, min_area, px_per_um, per_image_rows, all_props, writers=None,
              density=None, split_depth=None, shape=None, gt=None, clean=None, sweep=None, tta=None):
    batch = torch.stack(tensors).to(DEVICE)
    if tta is None:
        probs = model(batch)                             # sigmoid probabilities (model_2.py:80)
    elif batch.is_cuda:                                  # --tta: the mean over the variants, tta["batch"] items per forward
        from unet_dc_segmentation_amd.tta import predict_tta
        probs = predict_tta(model, batch, tta["N"], tta["batch"])
    else:
        from utils.tta import predict_tta_cpu
        probs = predict_tta_cpu(model, batch, tta["N"], tta["batch"])
    finish_batch(probs, meta, mask_dir, overlay_dir, thresh, min_area, px_per_um, per_image_rows, all_props, writers, density,
                 split_depth, shape, gt, clean, sweep)


def finish_batch(probs, meta, mask_dir, overlay_dir, thresh, min_area, px_per_um, per_image_rows, all_props, writers=None,
                 density=None, split_depth=None, shape=None, gt=None, clean=None, sweep=None):
    """Everything behind the forward: probs [B, 1, ph, pw] (on the device or not) -> masks of the sizes in meta, droplet tables,
    the optional stages and the per-image files.  run_batch feeds it the network-size maps, --tile one native-size map per image
    (ph, pw equal to the image's size: every resize rule is then the identity)."""
    on_device = probs.is_cuda
    if sweep is not None:                                # --thresh_sweep: the raw mask at every threshold, pooled
        sweep_step(sweep, probs, meta, gt, min_area, split_depth, clean)
    masks512 = None if on_device else (probs[:, 0] > thresh).to(torch.uint8).numpy()
    weak512 = None                                       # --prob_thresh_low on the CPU path: the mask of the low threshold
    if clean is not None and clean["low"] is not None and not on_device:
        weak512 = (probs[:, 0] > clean["low"]).to(torch.uint8).numpy()
    clean_counts = []
    if on_device:                                        # the whole batch enqueued back to back, ONE host wait (droplets.py)
        from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
        split = {} if split_depth is None else {"split_depth": split_depth, "return_labels": True}
        if shape is not None:                            # the grey planes go up behind the network's launches
            split.update(shape=True, gray=[torch.from_numpy(g).to(DEVICE) for g in shape["grays"]])
        if gt is not None and split_depth is None:       # the label maps come through the shape route; its rows may go unused
            split.update(shape=True, return_labels=True)
        if clean is not None:                            # the counts ride in the copy of the droplet counts
            split.update(thresh_low=clean["low"], max_hole_area=clean["holes"], clean_counts=clean_counts)
        if density is None:
            dev_out = mask_and_droplets_batch(probs[:, 0], thresh, [m[1] for m in meta], min_area, **split)
        else:                                            # the maps count every component: the table's sums serve when min_area <= 1
            from unet_dc_segmentation_amd.density import density_maps_batch
            dev_out, sums = mask_and_droplets_batch(probs[:, 0], thresh, [m[1] for m in meta], min_area, keep_sums=True, **split)
            # ... and when the table is not one of split droplets: the maps keep counting connected components
            dres = density_maps_batch(density["rgbs"], [o[0] for o in dev_out], sums if min_area <= 1 and not split else None,
                                      density["nb_layers"], density["kernel"])
        if gt is not None:                               # the batch's annotations against its label maps: one more host wait
            from unet_dc_segmentation_amd.evaluate import match_batch
            mres = match_batch([o[4] for o in dev_out], [o[1] for o in dev_out], gt["items"], gt["min_area"], gt["labels"])
    for i in range(len(meta)):
        fpath, (oh, ow) = meta[i]
        name = Path(fpath).stem
        labels = None
        if on_device:
            mask_d, area, cy, cx = dev_out[i][:4]
            mask, df = mask_d.cpu().numpy(), _droplet_table(area, cy, cx, px_per_um)
            if split_depth is not None:
                labels = dev_out[i][4].cpu().numpy()
            if shape is not None:
                df = add_shape_columns(df, dev_out[i][-1], (oh, ow), px_per_um)
        else:
            mask = resize_mask_like_reference(masks512[i], ow, oh)
            if clean is not None:                        # both masks under the same resize rule, then utils/droplet_clean.py
                from utils.droplet_clean import clean_mask
                weak = None if weak512 is None else resize_mask_like_reference(weak512[i], ow, oh)
                mask, counts = clean_mask(mask, weak, clean["holes"])
                clean_counts.append(counts)
            if shape is not None:
                df, labels = quantify_shape(mask, min_area, px_per_um, split_depth, shape["grays"][i])
            elif split_depth is None:
                df = quantify(mask, min_area, px_per_um)
            else:
                df, labels = quantify_split(mask, min_area, px_per_um, split_depth)
        if gt is not None:
            if on_device:
                res = mres[i]
            else:
                plab = labels if labels is not None else pred_labels_cpu(mask, min_area, split_depth)
                res = match_cpu(plab, df["area"].to_numpy() if not df.empty else np.zeros(0, np.int64), gt["items"][i],
                                gt["min_area"], gt["labels"])
            df = add_match_outputs(gt, df, res, Path(fpath).name)
        if clean is not None:
            from utils.droplet_clean import COUNT_NAMES
            clean["rows"].append({"filename": Path(fpath).name, **{k: int(v) for k, v in zip(COUNT_NAMES, clean_counts[i])}})
        df.insert(0, "filename", Path(fpath).name) if not df.empty else None
        all_props.append(df)
        per_image_rows.append({"filename": Path(fpath).name, "droplet_count": len(df),
                               "total_area_px": df["area"].sum() if not df.empty else 0})
        # PNG deflate and CSV formatting are the slowest part of an image once the network runs on the device: they go to
        # the writer pool (same files, same contents; main() waits for them before the summary is written)
        if writers is None:
            _write_outputs(mask, df, fpath, name, mask_dir, overlay_dir, labels)
        else:
            writers[1].append(writers[0].submit(_write_outputs, mask, df, fpath, name, mask_dir, overlay_dir, labels))
        if density is not None:
            _density(density, dres[i] if on_device else None, density["rgbs"][i], mask, fpath, name, writers)
        if writers is not None:
            # back-pressure: at most ~4 batches of masks / tables wait for the writers; waiting on the OLDEST write also surfaces a
            # failed write while the run is still going
            while len(writers[1]) > writers[2]:
                writers[1].popleft().result()


def build_parser():
    p = argparse.ArgumentParser("Segment lipid droplets and build a report")
    p.add_argument("--img_dir", required=True)
    p.add_argument("--ckpt_path", default="best_UNetDC_focal_model.pth")
    p.add_argument("--out_dir", default="quant_results")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--prob_thresh", type=float, default=0.3)
    p.add_argument("--min_area", type=int, default=1, help="ignore objects smaller than this (pixels^2)")
    p.add_argument("--px_per_micron", type=float, help="pixels per micron for physical-unit columns")
    p.add_argument("--save_overlays", action="store_true")
    p.add_argument("--background_radius", type=int, default=50, help="radius for rolling ball background correction")
    p.add_argument("--skip_excel", action="store_true", help="skip generation of the Excel workbook")
    p.add_argument("--skip_histogram", action="store_true", help="skip histogram plot generation")
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="compute type of the HIP path")
    p.add_argument("--density_maps", action="store_true",
                   help="also write radial / spatial droplet density heat maps and density_per_image.csv")
    p.add_argument("--nb_layers", type=int, default=10, help="concentric rings of the radial density map")
    p.add_argument("--density_kernel", type=int, default=21, help="spatial density Gaussian: sigma = density_kernel / 6")
    p.add_argument("--split_touching", action="store_true",
                   help="count touching droplets separately: cut every connected component where its distance transform dips "
                        "more than --split_depth below the lower of two peaks; also writes predicted_masks/NAME_labels.png "
                        "(16-bit label image).  The --density_maps outputs keep counting connected components")
    p.add_argument("--droplet_shape", action="store_true",
                   help="add shape and intensity columns to the droplet tables: perimeter, circularity, major / minor axis, "
                        "eccentricity, orientation, bounding box, touches_border, and mean / min / max / std of the original "
                        "image (as grey) under each droplet")
    p.add_argument("--gt_dir", help="score the droplets against annotated masks: the mask of NAME.ext is GT_DIR/NAME.<image "
                                    "suffix>, read as grey > 0 and labelled by 4-connected components (never split); adds "
                                    "gt_label / gt_iou / gt_covered to the droplet tables, writes gt_droplets.csv and "
                                    "match_per_image.csv")
    p.add_argument("--gt_min_area", type=int, default=1, help="ignore annotated objects smaller than this (pixels^2)")
    p.add_argument("--gt_labels", action="store_true",
                   help="the files of --gt_dir are label images (the 16-bit NAME_labels.png of --split_touching, or any integer "
                        "image): their values are the labels as they are, numbered 1..max (--gt_min_area does not apply)")
    p.add_argument("--prob_thresh_low", type=float,
                   help="hysteresis threshold: also keep every 4-connected region above this lower threshold that contains a "
                        "pixel above --prob_thresh (must not exceed it; equal = off)")
    p.add_argument("--fill_holes", type=int, nargs="?", const=-1, default=0, metavar="N",
                   help="fill the holes of the mask (background not 4-connected to the image border) before anything is "
                        "measured: holes of at most N pixels, of any size without N; writes mask_clean_per_image.csv")
    p.add_argument("--thresh_sweep", type=int, nargs="?", const=100, metavar="K",
                   help="with --gt_dir: score the thresholded mask against the annotation, pixel by pixel, at the K thresholds "
                        "k / K (K in 1..1024, 100 without K) in one pass per image, and write threshold_sweep.csv pooled over all "
                        "images (tp, fp, fn, tn, precision, recall, dice, iou per threshold).  It describes the raw mask "
                        "probs > threshold under the script's resize rule: --prob_thresh_low, --fill_holes, --min_area and "
                        "--gt_min_area do not enter it (a pixel score; with --gt_labels any nonzero label is annotated)")
    p.add_argument("--sweep_objects", metavar="T[,T...]",
                   help="with --thresh_sweep: run the droplet stage (with this run's split and cleaning options) and the "
                        "matching of --gt_dir again at each listed threshold, on the probabilities already computed, and write "
                        "threshold_sweep_objects.csv: the pooled row of match_per_image.csv per threshold (none may lie below "
                        "--prob_thresh_low)")
    p.add_argument("--tile", type=int, nargs="?", const=512, metavar="T",
                   help="run the network at the image's native resolution: cut the background-corrected image into overlapping "
                        "T x T tiles (T a multiple of 16 in 32..4096, 512 without T), forward them --batch at a time and blend "
                        "their probabilities into one map of the image's size; for checkpoints trained at that scale")
    p.add_argument("--tile_overlap", type=int, metavar="O",
                   help="with --tile: least overlap of neighbouring tiles in pixels, also the width of the blend ramp "
                        "(0..T/2, default 64)")
    p.add_argument("--tta", type=int, nargs="?", const=8, metavar="N",
                   help="test-time augmentation: run the network on N flipped and rotated variants of every input (of every "
                        "tile with --tile), map the outputs back and average them (N = 2: + horizontal flip, 4: the flips and "
                        "the half turn, 8: all flips and quarter turns; 8 without N); --batch stays the number of items per "
                        "forward")
    p.add_argument("--split_depth", type=float, default=2.0,
                   help="depth of the dip, in pixels, that separates two droplets under --split_touching (a multiple of 0.5)")
    return p


def clean_options(args):
    """--prob_thresh_low / --fill_holes -> {"low": threshold or None, "holes": limit (-1 = any size), "rows": []}, None with
    both off; a bad value ends the run before any image."""
    low, holes = args.prob_thresh_low, args.fill_holes
    if low is not None and not low <= args.prob_thresh:
        raise SystemExit(f"--prob_thresh_low ({low}) must not exceed --prob_thresh ({args.prob_thresh})")
    if holes < -1:
        raise SystemExit("--fill_holes N: N is a number of pixels (0 = off)")
    if low is not None and low == args.prob_thresh:
        low = None                                       # selects what --prob_thresh selects
    return None if low is None and holes == 0 else {"low": low, "holes": holes, "rows": []}


def sweep_options(args):
    """--thresh_sweep / --sweep_objects -> {"K", "hist", "objects", "object_images"}, None without the flag; a bad value or
    a missing --gt_dir ends the run before any image."""
    if args.thresh_sweep is None:
        if args.sweep_objects is not None:
            raise SystemExit("--sweep_objects needs --thresh_sweep")
        return None
    if not args.gt_dir:
        raise SystemExit("--thresh_sweep scores against annotated masks: it needs --gt_dir")
    from utils.threshold_sweep import MAX_K
    if not 1 <= args.thresh_sweep <= MAX_K:
        raise SystemExit(f"--thresh_sweep K: K must be in 1..{MAX_K}")
    objects = []
    if args.sweep_objects is not None:
        try:
            objects = [float(v) for v in args.sweep_objects.split(",") if v.strip()]
        except ValueError:
            raise SystemExit("--sweep_objects takes thresholds separated by commas, e.g. 0.2,0.3,0.4")
        low = args.prob_thresh_low
        for t in objects:
            if not t == t or (low is not None and t < low):
                raise SystemExit(f"--sweep_objects: {t} lies below --prob_thresh_low ({low})")
        objects = list(dict.fromkeys(objects))
    return {"K": args.thresh_sweep, "hist": None, "objects": objects, "object_images": {t: [] for t in objects}}


def tile_options(args):
    """--tile / --tile_overlap -> {"T", "O"}, None without --tile; a bad value ends the run before any image."""
    if args.tile is None:
        if args.tile_overlap is not None:
            raise SystemExit("--tile_overlap needs --tile")
        return None
    from utils.tiling import check_tile
    try:
        T, O = check_tile(args.tile, 64 if args.tile_overlap is None else args.tile_overlap)
    except ValueError as e:
        raise SystemExit(f"--tile / --tile_overlap: {e}")
    if args.batch < 1:
        raise SystemExit("--tile: --batch is the number of tiles per forward, at least 1")
    return {"T": T, "O": O}


def tta_options(args):
    """--tta -> {"N", "batch"}, None without the flag or with N = 1 (the identity alone: the plain forward); a bad value ends
    the run before any image."""
    if args.tta is None:
        return None
    from utils.tta import TTA_SIZES
    if args.tta not in TTA_SIZES:
        raise SystemExit(f"--tta N: N must be one of {', '.join(map(str, TTA_SIZES))}, not {args.tta}")
    if args.batch < 1:
        raise SystemExit("--tta: --batch is the number of items per forward, at least 1")
    return None if args.tta == 1 else {"N": args.tta, "batch": args.batch}


def main(argv=None):
    args = build_parser().parse_args(argv)
    in_dir, out_dir = Path(args.img_dir), Path(args.out_dir)
    from utils.droplet_split import half_pixels
    try:                                                 # checked before any image, and before any output directory exists
        split_depth = half_pixels(args.split_depth) / 2.0
    except ValueError:
        raise SystemExit("--split_depth must be a non-negative multiple of 0.5")
    if not args.split_touching:
        split_depth = None
    clean = clean_options(args)
    sweep = sweep_options(args)
    tile = tile_options(args)
    tta = tta_options(args)
    images = sorted(p for p in in_dir.iterdir() if p.suffix.lower() in IMAGE_SUFFIXES)
    gt = None
    if args.gt_dir:                                      # every annotation is there and of its image's size, or nothing runs
        gt = {"files": find_gt_files(images, args.gt_dir), "min_area": args.gt_min_area, "labels": args.gt_labels, "items": [],
              "tables": [], "images": []}
    mask_dir = out_dir / "predicted_masks"
    overlay_dir = out_dir / "overlays" if args.save_overlays else None
    out_dir.mkdir(parents=True, exist_ok=True)
    mask_dir.mkdir(exist_ok=True)
    if overlay_dir:
        overlay_dir.mkdir(exist_ok=True)
    density = None
    if args.density_maps:
        # the limits of the device path (UNETDC_DENSITY_MAX_LAYERS, UNETDC_DENSITY_MAX_RADIUS), checked before any image on
        # either path: the Gaussian radius int(4 sigma + 0.5), sigma = density_kernel / 6, is at most 128
        if not 1 <= args.nb_layers <= 255 or not 0 < args.density_kernel or int(4 * args.density_kernel / 6 + 0.5) > 128:
            raise SystemExit("--nb_layers must be in 1..255 and --density_kernel in 1..192")
        density = {"nb_layers": args.nb_layers, "kernel": args.density_kernel, "rows": [], "rgbs": [], "out_dir": out_dir}
    shape = {"grays": []} if args.droplet_shape else None
    model = load_model(args.ckpt_path, args.dtype)
    tensors, meta, per_image_rows, all_props = [], [], [], []
    # File decode runs ahead of the device and the per-image writes behind it, in two small thread pools (both are
    # zlib-bound and release the GIL); the order of the rows in the summary files is the order of `images` as before.
    import os
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    nthreads = max(1, min(8, (os.cpu_count() or 2) // 2))
    with ThreadPoolExecutor(nthreads) as dec_pool, ThreadPoolExecutor(nthreads) as wr_pool:
        writers = (wr_pool, deque(), 4 * max(1, args.batch))
        ahead = deque()
        it = iter(images)

        def refill():
            while len(ahead) < 2 * args.batch:
                nxt = next(it, None)
                if nxt is None:
                    return
                ahead.append((nxt, dec_pool.submit(decode_rgb, nxt),
                              None if gt is None else dec_pool.submit(decode_gt, gt["files"][str(nxt)], gt["labels"])))

        refill()
        while ahead:
            img, fut, gt_fut = ahead.popleft()
            refill()
            im = fut.result()
            if shape is not None:                        # the ORIGINAL image as grey, before the rolling ball
                from utils.density import rgb_to_gray
                shape["grays"].append(rgb_to_gray(im))
            if tile is not None:                         # native size: one map per image, the stages on a batch of one
                if gt is not None:
                    gt["items"].append(gt_fut.result())
                probs, rgb = predict_tiled_image(model, im, args.background_radius, tile, args.batch, density is not None, tta)
                if density is not None:
                    density["rgbs"] = [rgb]
                finish_batch(probs, [(str(img), im.shape[:2])], mask_dir, overlay_dir, args.prob_thresh, args.min_area,
                             args.px_per_micron, per_image_rows, all_props, writers, density, split_depth, shape, gt, clean, sweep)
                if shape is not None:
                    shape["grays"] = []
                if gt is not None:
                    gt["items"] = []
                continue
            if density is None:
                t, osize = preprocess(img, args.background_radius, im)
            else:
                t, osize, rgb = preprocess(img, args.background_radius, im, keep_rgb=True)
                density["rgbs"].append(rgb)
            if gt is not None:
                gt["items"].append(gt_fut.result())
            tensors.append(t)
            meta.append((str(img), osize))
            if len(tensors) == args.batch:
                run_batch(tensors, meta, model, mask_dir, overlay_dir, args.prob_thresh, args.min_area,
                          args.px_per_micron, per_image_rows, all_props, writers, density, split_depth, shape, gt, clean, sweep, tta)
                tensors, meta = [], []
                if density is not None:
                    density["rgbs"] = []
                if shape is not None:
                    shape["grays"] = []
                if gt is not None:
                    gt["items"] = []
        if tensors:
            run_batch(tensors, meta, model, mask_dir, overlay_dir, args.prob_thresh, args.min_area,
                      args.px_per_micron, per_image_rows, all_props, writers, density, split_depth, shape, gt, clean, sweep, tta)
        for f in writers[1]:
            f.result()                                   # re-raises a failed write
    if density is not None:
        pd.DataFrame(density["rows"]).to_csv(out_dir / "density_per_image.csv", index=False)
    if gt is not None:
        from utils.droplet_match import pooled_row, summary_row
        tables = [t for t in gt["tables"] if len(t)] or gt["tables"][:1]
        pd.concat(tables, ignore_index=True).to_csv(out_dir / "gt_droplets.csv", index=False) if tables else None
        rows = [summary_row(name, ints) for name, ints in gt["images"]] + [pooled_row([ints for _, ints in gt["images"]])]
        pd.DataFrame(rows).to_csv(out_dir / "match_per_image.csv", index=False)
    if clean is not None:
        pd.DataFrame(clean["rows"]).to_csv(out_dir / "mask_clean_per_image.csv", index=False)
    if sweep is not None and sweep["hist"] is not None:
        from utils.threshold_sweep import summary_line, table_rows
        hist = sweep["hist"]
        if torch.is_tensor(hist):                        # the sweep's only copy from the device
            from unet_dc_segmentation_amd.evaluate import sweep_result
            hist = sweep_result(hist)
        pd.DataFrame(table_rows(hist)).to_csv(out_dir / "threshold_sweep.csv", index=False)
        print(summary_line(hist))
        if sweep["objects"]:
            from utils.droplet_match import pooled_row
            rows = []
            for t in sweep["objects"]:
                row = pooled_row(sweep["object_images"][t])
                row.pop("filename")
                rows.append({"threshold": t, **row})
            pd.DataFrame(rows).to_csv(out_dir / "threshold_sweep_objects.csv", index=False)
    summary_df = pd.DataFrame(per_image_rows)
    summary_df.to_csv(out_dir / "summary_per_image.csv", index=False)
    props = [d for d in all_props if not d.empty]
    if props:
        combined = pd.concat(props, ignore_index=True)
        combined.to_csv(out_dir / "all_droplets.csv", index=False)
        if not args.skip_excel:
            try:
                import xlsxwriter  # noqa: F401
                with pd.ExcelWriter(out_dir / "all_droplets.xlsx", engine="xlsxwriter") as xw:
                    combined.to_excel(xw, index=False, sheet_name="droplets")
                    summary_df.to_excel(xw, index=False, sheet_name="per_image")
            except (ImportError, AttributeError):
                combined.to_csv(out_dir / "all_droplets_noexcel.csv", index=False)
                print("Skipped Excel file (xlsxwriter not available); wrote all_droplets_noexcel.csv")
        size_col = "eq_diam_micron" if "eq_diam_micron" in combined.columns else "equivalent_diameter"
        stats = combined[size_col].describe()[["mean", "50%", "std"]].rename({"50%": "median"})
        stats.to_csv(out_dir / "droplet_size_stats.csv")
        if not args.skip_histogram:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            plt.figure(figsize=(6, 4))
            plt.hist(combined[size_col], bins=40)
            plt.xlabel("Diameter (um)" if "micron" in size_col else "Diameter (pixels)")
            plt.ylabel("Count")
            plt.title("Droplet size distribution")
            plt.tight_layout()
            plt.savefig(out_dir / "size_histogram.png", dpi=300)
            plt.close()
    print("\n All done. Outputs are in ", out_dir)
    return out_dir


if __name__ == "__main__":
    main()
