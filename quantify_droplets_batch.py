#!/usr/bin/env python3
"""Batch inference + droplet quantification -- drop-in for the reference's ``quantify_droplets_batch.py`` (same CLI
flags: the Tk/Qt front-ends build this argv, gui.py:26-39, gui_qt.py:372-400; same output files and CSV columns,
outputs/all_droplets.csv:1).  ``--help`` describes every flag, DESIGN.md sections 10 to 17 every stage.

main() validates the options into one Run, then per batch: decode and preprocess (rolling ball, resize to 512, /255) ->
run_batch (the network; --tta averages it over flips and rotations; --tile runs it on native-size tiles instead and blends
them) -> finish_batch (threshold, resize of the mask to the image's size, optional cleaning, components or split droplets,
tables, optional shape columns, matching against annotations, threshold sweep, density maps, the per-image files) -> the
summary files.  With a GPU (``DEVICE = "cuda"``) every stage behind the decode runs in HIP kernels and only the uint8 mask
and a few integers per droplet come back:

    preprocessing     unet_dc_segmentation_amd/preprocess.py    csrc/preprocess.hip     CPU: utils/data_loader.py
    tiles, blend      unet_dc_segmentation_amd/tiling.py        csrc/tile.hip           CPU: utils/tiling.py
    --tta             unet_dc_segmentation_amd/tta.py           csrc/tta.hip            CPU: utils/tta.py
    mask, droplets    unet_dc_segmentation_amd/droplets.py      csrc/ccl.hip            CPU: droplets_cpu() here (SciPy)
    cleaning, split   (droplets.py)                             csrc/clean.hip split.hip  CPU: utils/droplet_clean.py, droplet_split.py
    shape columns     (droplets.py)                             csrc/shape.hip          CPU: utils/droplet_shape.py
    --gt_dir, sweep   unet_dc_segmentation_amd/evaluate.py      csrc/match.hip sweep.hip  CPU: utils/droplet_match.py, threshold_sweep.py
    --density_maps    unet_dc_segmentation_amd/density.py       csrc/density.hip        CPU: utils/density.py
    --neighbors       (droplets.py)                             csrc/neighbors.hip      CPU: utils/droplet_neighbors.py
    --boundary        unet_dc_segmentation_amd/evaluate.py      csrc/boundary.hip       CPU: utils/droplet_boundary.py
    --confidence      (droplets.py, tta.py)                     csrc/confidence.hip tta.hip  CPU: utils/droplet_confidence.py
    --droplet_hull    (droplets.py)                             csrc/hull.hip           CPU: utils/droplet_hull.py
    --diff_maps       unet_dc_segmentation_amd/evaluate.py      csrc/diffmap.hip        CPU: utils/difference_map.py
    --outlines        unet_dc_segmentation_amd/outlines.py      csrc/outlines.hip       CPU: utils/droplet_outlines.py
    --spatial_stats   unet_dc_segmentation_amd/spatial.py       csrc/spatial.hip        CPU: utils/spatial_stats.py
    --gt_polygons     unet_dc_segmentation_amd/polygons.py      csrc/polyfill.hip       CPU: utils/polygon_masks.py
    --cell_dir, --nuclei_dir  unet_dc_segmentation_amd/cells.py (droplets.py)  csrc/cells.hip  CPU: utils/droplet_cells.py
    --intensity_window, --intensity_levels (in front of the preprocessing)
                      unet_dc_segmentation_amd/window.py        csrc/window.hip         CPU: utils/intensity_window.py

Without a GPU the network runs on PyTorch-CPU like the reference, and every stage has one derivation shared with the
device.  The mask's resize reproduces what the reference's call computes (droplets.py:MASK_RESIZE).
"""
import argparse
import dataclasses
from pathlib import Path

import numpy as np
import pandas as pd
import torch
from PIL import Image

from models.model_2 import UNetDC
from unet_dc_segmentation_amd.droplets import DropletOptions, Droplets, resize_mask_like_reference
from utils import intensity_window as iw
from utils.data_loader import resize_image, rolling_ball_correction_rgb

DEVICE = "cuda" if torch.cuda.is_available() else "cpu"
IMG_SIZE = 512          # matches the training resize


def load_model(ckpt, dtype="f32"):
    m = UNetDC(in_channels=3, out_channels=1)
    m.load_state_dict(torch.load(ckpt, map_location=DEVICE, weights_only=True))
    m.set_compute_dtype(dtype)
    return m.to(DEVICE).eval()


def decode_rgb(path):
    """File -> uint8 RGB array (runs in the decode pool: PIL releases the GIL while it inflates).  A deep image is clipped at
    255 by convert("RGB"): the first one of a run is reported, with the flag that windows it instead."""
    return iw.decode_rgb_clipped(path)


def decode_image(path, intensity=None):
    """The decode pool's job: the RGB array, or with a window flag (uint16 [h, w, c], the file's mode) for window_image."""
    if intensity is None:
        return decode_rgb(path)
    return iw.decode_deep_info(path, intensity["spec"].page)


def window_image(run, path, arr, mode):
    """--intensity_window / --intensity_levels: decoded uint16 image -> the 8-bit RGB image every later stage takes as 'the
    original' (a device tensor on the GPU path, where nothing comes back before the summary), and its record for
    intensity_per_image.csv."""
    spec = run.intensity["spec"]
    if DEVICE == "cuda":
        from unet_dc_segmentation_amd.window import deep_to_u8_device
        u8, rec = deep_to_u8_device(arr, spec, DEVICE)
    else:
        u8, rec = iw.deep_to_u8_numpy(arr, spec)
    run.intensity["records"].append((Path(path).name, mode, arr.shape[0] * arr.shape[1], rec))
    return u8


def preprocess(path, background_radius, im=None, keep_rgb=False):
    """-> (network input, (oh, ow)), and with keep_rgb the decoded original image as well (a device tensor on the GPU
    path: the density maps read it there without a second upload)."""
    im = decode_rgb(path) if im is None else im
    oh, ow = im.shape[:2]
    if DEVICE == "cuda":                                 # rolling ball + resize + /255 + CHW on the GPU (csrc/preprocess.hip)
        from unet_dc_segmentation_amd.preprocess import preprocess_device, preprocess_device_u8
        if torch.is_tensor(im):                          # the windowed image is on the device already
            x = preprocess_device_u8(im, background_radius, IMG_SIZE, return_rgb=keep_rgb)
            return (x[0], (oh, ow), x[1]) if keep_rgb else (x, (oh, ow))
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


@dataclasses.dataclass
class Run:
    """One invocation: the validated options, where the outputs go, and what accumulates over the images.  Built once in
    main(); nothing in it belongs to a single batch."""
    thresh: float
    min_area: int
    px_per_um: float | None
    background_radius: int
    batch_size: int
    split_depth: float | None          # --split_touching: the depth in pixels, None without the flag
    shape: bool                        # --droplet_shape
    clean: dict | None                 # clean_options(); its "rows" collect mask_clean_per_image.csv
    sweep: dict | None                 # sweep_options(); its "hist" / "object_images" collect the sweep's tables
    tile: dict | None                  # tile_options()
    tta: dict | None                   # tta_options()
    density: dict | None               # --density_maps: {"nb_layers", "kernel"}
    gt: dict | None                    # --gt_dir: {"files", "min_area", "labels"}; --gt_polygons: "polygons" in place of "files"
    out_dir: Path
    mask_dir: Path
    overlay_dir: Path | None
    writers: tuple                     # (writer pool, deque of pending writes, how many may be pending)
    rows: list = dataclasses.field(default_factory=list)           # summary_per_image.csv
    tables: list = dataclasses.field(default_factory=list)         # all_droplets.csv, one table per image
    density_rows: list = dataclasses.field(default_factory=list)   # density_per_image.csv
    gt_tables: list = dataclasses.field(default_factory=list)      # gt_droplets.csv, one table per image
    gt_images: list = dataclasses.field(default_factory=list)      # match_per_image.csv: (filename, integers)
    neighbors: int | None = None       # --neighbors: the contact radius in pixels
    contact_tables: list = dataclasses.field(default_factory=list)  # droplet_contacts.csv, one table per image
    boundary: dict | None = None       # boundary_options(); its "records" collect boundary_per_image.csv
    confidence: dict | None = None     # confidence_options(); its "rows" collect confidence_per_image.csv
    hull: float | None = None          # --droplet_hull: the solidity below which a droplet is flagged, None without the flag
    diff: dict | None = None           # diff_options(); its "tables" / "rows" collect diff_regions.csv and diff_regions_per_image.csv
    spatial: dict | None = None        # spatial_options(); its "table" / "rows" collect spatial_stats.csv and spatial_per_image.csv
    outlines: dict | None = None       # --outlines: {"dir", "images", "jobs"}: outlines/NAME.geojson and what outlines_coco.json collects
    intensity: dict | None = None      # --intensity_window / --intensity_levels: {"spec", "records"}: intensity_per_image.csv
    cells: dict | None = None          # built in main(): the flags, the files; its "tables" / "rows" collect cells.csv and cells_per_image.csv

    @property
    def keep_rgb(self):
        """Whether the batch keeps the decoded original image: the density maps read it, the difference overlays are painted on it."""
        return self.density is not None or self.diff is not None or (self.intensity is not None and self.overlay_dir is not None)

    @property
    def envelope(self):
        """Whether the forward also keeps the minimum and maximum over the variants: only with both --tta and --confidence."""
        return self.tta is not None and self.confidence is not None

    def droplet_options(self, labels, shape, confidence=False, hull=False, cells=False):
        """The device droplet stage of this run.  Without a split depth the label map comes from the labelling of the shape
        route (unetdc_ccl_labels), so asking for labels selects that route, unless a stage that reads the label map
        (DropletOptions.label_map) has selected it already."""
        c = self.clean or {"low": None, "holes": 0}
        conf = self.confidence if confidence else None
        opts = DropletOptions(split_depth=self.split_depth, shape=shape, thresh_low=c["low"], max_hole_area=c["holes"],
                              neighbors=self.neighbors, confidence=None if conf is None else conf["band"],
                              confidence_maps=conf is not None and conf["maps"], hull=hull, cells=cells)
        route = labels and self.split_depth is None and not opts.label_map
        return dataclasses.replace(opts, labels=labels, shape=shape or route)

    def submit(self, fn, *args):
        """PNG deflate and CSV formatting are the slowest part of an image once the network runs on the device: they go to
        the writer pool (main() waits for them before the summary is written)."""
        self.writers[1].append(self.writers[0].submit(fn, *args))


@dataclasses.dataclass
class Batch:
    """What one forward and the stages behind it read, made fresh for every batch: entry i of every list is image i."""
    meta: list = dataclasses.field(default_factory=list)       # (path, (oh, ow))
    tensors: list = dataclasses.field(default_factory=list)    # network inputs (none under --tile)
    grays: list = dataclasses.field(default_factory=list)      # --droplet_shape: the ORIGINAL image as grey, uint8 [oh, ow]
    rgbs: list = dataclasses.field(default_factory=list)       # --density_maps, --diff_maps: the decoded image (a device tensor on the GPU)
    gt_items: list = dataclasses.field(default_factory=list)   # --gt_dir: the decoded annotations
    windows: list = dataclasses.field(default_factory=list)    # --spatial_window_dir: the decoded windows, uint8 {0, 1}
    cells: list = dataclasses.field(default_factory=list)      # --cell_dir / --nuclei_dir: the decoded (label map, ids), then (cell_maps) the cells
    cell_ids: list = dataclasses.field(default_factory=list)   # per image the file's own cell numbers, None where they are 1..K already


def predict_tiled_image(model, im, run):
    """--tile: decoded image -> (probabilities [1, 1, H, W] at the image's own size, the original image for the density maps or
    None); with --tta and --confidence the probabilities are the triple (mean, lo, hi) of that shape.  Preprocessing is the
    rolling ball alone, at native size; then the tiles, run.batch_size per forward, and the blend.  With --tta every tile's
    probabilities are the mean over its variants."""
    more = {} if run.tta is None else {"tta": run.tta["N"], "envelope": True} if run.envelope else {"tta": run.tta["N"]}
    tile, radius, keep_rgb = run.tile, run.background_radius, run.keep_rgb
    if DEVICE == "cuda":
        from unet_dc_segmentation_amd.preprocess import MAX_ELEMENT, _upload, rolling_ball_device
        from unet_dc_segmentation_amd.tiling import predict_tiled
        host_ball = int(radius) > MAX_ELEMENT                # the element does not fit the kernel's LDS tile: host operator
        rgb = _upload(im, DEVICE) if keep_rgb or not host_ball else None
        corrected = (_upload(rolling_ball_correction_rgb(im, int(radius)), DEVICE) if host_ball
                     else rolling_ball_device(rgb, radius))
        p = predict_tiled(model, corrected, tile["T"], tile["O"], run.batch_size, **more)
        return (tuple(q[None, None] for q in p) if run.envelope else p[None, None]), rgb
    from utils.tiling import predict_tiled_cpu
    p = predict_tiled_cpu(model, rolling_ball_correction_rgb(im, radius), tile["T"], tile["O"], run.batch_size, **more)
    return (tuple(torch.from_numpy(q)[None, None] for q in p) if run.envelope else torch.from_numpy(p)[None, None]), (im if keep_rgb else None)


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


def add_shape_columns(df, props, hw, px_per_um):
    """--droplet_shape: the columns of utils.droplet_shape.shape_columns behind the table's own."""
    if df.empty:
        return df
    from utils.droplet_shape import shape_columns
    for name, col in shape_columns(props, hw, px_per_um).items():
        df[name] = col
    return df


def _components(bin_mask, min_area):
    """(area, centroid_row, centroid_col) of the 4-connected components of at least min_area pixels, in label order (SciPy:
    ``ndimage.label`` with its default cross-shaped structure is skimage's ``label(connectivity=1)``)."""
    from scipy import ndimage
    lbl, n = ndimage.label(bin_mask)                     # 4-connectivity, labels in raster order of the first pixel
    if n:
        areas = np.bincount(lbl.ravel(), minlength=n + 1)
        keep = areas >= min_area
        keep[0] = False
        lbl, n = ndimage.label(keep[lbl])
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    area = np.bincount(lbl.ravel(), minlength=n + 1)[1:]
    cen = np.array(ndimage.center_of_mass(np.ones_like(lbl), lbl, np.arange(1, n + 1))).reshape(n, 2)
    return area, cen[:, 0], cen[:, 1]


def droplets_cpu(bin_mask, min_area, split_depth=None, shape=False, gray=None, labels=False, neighbors=None, confidence=None, hull=False,
                 cells=None):
    """CPU path: the record that droplets.mask_and_droplets_batch returns per image, in host arrays, from the uint8 mask at
    the image's size.  split_depth: the split droplets (utils/droplet_split.py); shape: the integers of
    utils.droplet_shape.label_props_numpy on the label map and the grey plane, centroids then the integer sums over the
    area as on the device; labels: the int32 label map whose numbers are the rows of the table; neighbors (a radius): the
    record of utils.droplet_neighbors.neighbors_numpy on the label map, centroids from the integer sums as well; confidence
    (the keywords probs, thresh, band, lo, hi, maps of utils.droplet_confidence.confidence_numpy): its record on the label map;
    hull: the integers of utils.droplet_hull.label_hull_numpy on the label map; cells ((cell label map, its largest label, the d2
    plane or None), as cell_maps makes them): the record of utils.droplet_cells.cells_record on the label map."""
    lab, rec = None, {}
    label_map = shape or neighbors is not None or confidence is not None or hull or cells is not None   # a stage reads it, as DropletOptions.label_map
    if split_depth is not None:
        from utils.droplet_split import half_pixels, split_labels
        lab, area, sy, sx, _ = split_labels(bin_mask, half_pixels(split_depth), min_area)
    elif label_map or labels:
        from utils.droplet_match import gt_labels_numpy, label_sums
        lab = gt_labels_numpy(bin_mask, min_area)
        if label_map and not shape:                      # shape brings its own
            area, sy, sx = label_sums(lab)
    if split_depth is None and not label_map:
        area, cen_row, cen_col = _components(bin_mask, min_area)
    else:                                                # then the stages, in the order of the device's
        if shape:
            from utils.droplet_shape import label_props_numpy
            rec["props"] = label_props_numpy(lab, gray)
            area, sy, sx = (rec["props"][q] for q in ("area", "Sy", "Sx"))
        if neighbors is not None:
            from utils.droplet_neighbors import neighbors_numpy
            rec["neighbors"] = neighbors_numpy(lab, len(area), neighbors)
        if confidence is not None:
            from utils.droplet_confidence import confidence_numpy
            rec["confidence"] = confidence_numpy(lab, max_out=len(area), **confidence)
        if hull:
            from utils.droplet_hull import label_hull_numpy
            rec["hull"] = label_hull_numpy(lab, len(area))
        if cells is not None:
            from utils.droplet_cells import cells_record
            rec["cells"] = cells_record(lab, len(area), *cells)
        d = np.maximum(area, 1)
        cen_row, cen_col = sy.astype(np.float64) / d, sx.astype(np.float64) / d
    more = {"cells": rec.pop("cells")} if "cells" in rec else {}
    return Droplets(bin_mask, area, cen_row, cen_col, labels=lab, **rec).with_records(**more)


def quantify_shape(bin_mask, min_area, px_per_um, split_depth, gray):
    """CPU path of --droplet_shape: (table with the shape columns, label map or None without a split depth)."""
    d = droplets_cpu(bin_mask, min_area, split_depth, True, gray)
    df = add_shape_columns(_droplet_table(d.area, d.centroid_row, d.centroid_col, px_per_um), d.props, bin_mask.shape, px_per_um)
    return df, (d.labels if split_depth is not None else None)


IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".tif", ".tiff")


def find_gt_files(images, gt_dir, flag="--gt_dir", what="annotated mask"):
    """--gt_dir: {image path: annotation path}, checked before anything runs.  The annotation of NAME.ext is
    gt_dir/NAME.<any image suffix>; a missing one, or one whose size differs from its image, ends the run (PIL reads the
    sizes from the headers, nothing is decoded).  --spatial_window_dir finds its windows by the same rule."""
    found = {}
    for img in images:
        cands = [q for q in sorted(Path(gt_dir).glob(img.stem + ".*")) if q.suffix.lower() in IMAGE_SUFFIXES and q.stem == img.stem]
        if not cands:
            raise SystemExit(f"{flag}: no {what} for {img.name} ({Path(gt_dir) / (img.stem + '.*')})")
        with Image.open(img) as a, Image.open(cands[0]) as b:
            if a.size != b.size:
                raise SystemExit(f"{flag}: {cands[0]} is {b.size[0]} x {b.size[1]}, its image {img.name} {a.size[0]} x {a.size[1]}")
        found[str(img)] = cands[0]
    return found


def find_gt_polygons(images, path):
    """--gt_polygons: {image path: load}, checked before anything runs (utils/polygon_masks.py).  A
    directory holds NAME.geojson per image; a .json file is COCO, its images matched by the stem of file_name.  A missing
    annotation or a COCO size that differs from the image ends the run here; the files are read and packed by
    decode_gt_polygons on the decode pool, ahead of the device like the files of --gt_dir."""
    from utils import polygon_masks as pm
    try:
        return pm.find_polygons(path, images)
    except pm.PolygonError as e:
        raise SystemExit(f"--gt_polygons: {e}")


def decode_gt_polygons(load):
    """One image's polygons -> (packed record, number of features); what the reader or pack refuses ends the run."""
    from utils.polygon_masks import PolygonError
    try:
        return load()
    except PolygonError as e:
        raise SystemExit(f"--gt_polygons: {e}")


def rasterize_gt(run, batch, on_device):
    """--gt_polygons: the packed polygons of the batch -> label maps of the images' sizes, numbered 1..K (what --gt_dir with
    --gt_labels decodes from files): DEVICE tensors through polygons.rasterize_batch when the run is on the device, else
    rasterize_numpy.  Features that own no pixel are dropped and counted."""
    gt, hws = run.gt, [m[1] for m in batch.meta]
    if on_device:
        from unet_dc_segmentation_amd.polygons import rasterize_batch
        recs = rasterize_batch([p for p, _ in batch.gt_items], hws, compact=True, device=DEVICE)
    else:
        from utils.polygon_masks import rasterize_numpy
        recs = [rasterize_numpy(p, *hw, compact=True) for (p, _), hw in zip(batch.gt_items, hws)]
    gt["features"] += sum(n for _, n in batch.gt_items)
    gt["dropped"] += sum(n - len(r["kept"]) for (_, n), r in zip(batch.gt_items, recs))
    batch.gt_items = [r["labels"] for r in recs]


def decode_gt(path, as_labels):
    """Annotation file -> uint8 {0, 1} mask (convert("L") > 0, as SegmentationDataset reads it) or, with --gt_labels, the
    int32 label image as it is."""
    im = Image.open(path)
    if not as_labels:
        return (np.array(im.convert("L")) > 0).astype(np.uint8)
    return np.array(im if im.mode in ("1", "L", "P", "I", "I;16", "I;16B") else im.convert("I")).astype(np.int32)


def match_cpu(labels, area, gt_item, gt_min_area, gt_are_labels, boundary=None):
    """CPU path of --gt_dir for one image: what unet_dc_segmentation_amd.evaluate.match_batch returns per image; with
    boundary (a radius) also the record of utils.droplet_boundary.boundary_record_numpy under "boundary"."""
    from utils import droplet_match as dm
    glab = gt_item if gt_are_labels else dm.gt_labels_numpy(gt_item, gt_min_area)
    garea, gsy, gsx = dm.label_sums(glab)
    a, b, n = dm.overlap_table_numpy(labels, glab, len(area), len(garea))
    res = {"a": a, "b": b, "n": n, "gt_area": garea, "gt_sumy": gsy, "gt_sumx": gsx,
           "columns": dm.match_columns(area, garea, a, b, n)}
    if boundary is not None:
        from utils.droplet_boundary import boundary_record_numpy
        res["boundary"] = boundary_record_numpy(labels, len(area), glab, len(garea), boundary)
    return res


def add_match_outputs(run, df, res, filename):
    """--gt_dir: the three columns behind the droplet table's own, this image's rows of gt_droplets.csv and its integers; with
    --boundary the per-object boundary columns and this image's record as well."""
    from utils.droplet_match import gt_table
    pred_cols, gt_cols = dict(res["columns"]["pred"]), dict(res["columns"]["gt"])
    if run.boundary is not None:                         # --boundary: bd_px, bd_rms, bd_max behind them, on both tables
        from utils.droplet_boundary import object_columns
        rec = res["boundary"]
        pred_cols.update(object_columns(rec["a"]))
        gt_cols.update(object_columns(rec["b"]))
        run.boundary["records"].append((filename, rec["hist"], rec["dmax"]))
    if not df.empty:
        for name, col in pred_cols.items():
            df[name] = col
    run.gt_tables.append(pd.DataFrame(gt_table(filename, res["gt_area"], res["gt_sumy"], res["gt_sumx"], gt_cols)))
    run.gt_images.append((filename, res["columns"]["image"]))
    return df


def add_neighbor_outputs(run, df, d, filename):
    """--neighbors: the columns behind the droplet table's own, this image's rows of droplet_contacts.csv -> (the table, the
    numbers its row of summary_per_image.csv gains)."""
    from utils import droplet_neighbors as dn
    rec = d.neighbors
    pairs = tuple(rec["pairs"][q] for q in ("a", "b", "d2"))
    if not df.empty:                                     # one concat: column by column costs six frame insertions per image
        cols = dn.table_columns(rec, d.centroid_row, d.centroid_col, run.px_per_um)
        df = pd.concat([df, pd.DataFrame(cols, index=df.index)], axis=1)
    run.contact_tables.append(pd.DataFrame(dn.contact_table(filename, pairs)))
    return df, dn.summary(pairs, rec)


def add_confidence_outputs(run, df, d, filename, name):
    """--confidence: the columns of utils.droplet_confidence.confidence_columns behind the droplet table's own, this image's row
    of confidence_per_image.csv, and with --confidence_maps the two map PNGs through the writer pool."""
    from utils import droplet_confidence as dc
    rec = d.confidence
    if not df.empty:
        df = pd.concat([df, pd.DataFrame(dc.confidence_columns(rec), index=df.index)], axis=1)
    run.confidence["rows"].append({"filename": filename, **dc.image_columns(rec)})
    for key, suffix in (("entropy_u8", "entropy"), ("spread_u8", "spread")):
        if rec.get(key) is not None:
            run.submit(_write_map, _host(rec[key]), run.out_dir / f"{name}_{suffix}.png")
    return df


def decode_cells(path, as_labels, min_area):
    """--cell_dir / --nuclei_dir: one mask file -> the int32 label map of its objects: with --cell_labels the label image as it
    is (decode_gt), else the 4-connected components of at least min_area pixels of the binary mask, numbered in raster order.
    -> (the map, ids): a label image whose ids have gaps (one object numbered 60000) is renumbered 1..K in ascending order, so that
    the per-cell buffers are sized by the cells there are, and ids [K] holds the file's own numbers for the tables; None otherwise."""
    item = decode_gt(path, as_labels)
    if not as_labels:
        from utils.droplet_match import gt_labels_numpy
        return gt_labels_numpy(item, min_area), None
    ids = np.unique(item[item > 0])
    if len(ids) == 0 or len(ids) == int(ids[-1]):
        return item, None
    return np.where(item > 0, np.searchsorted(ids, item) + 1, 0).astype(np.int32), ids.astype(np.int64)


def cell_maps(run, batch, on_device):
    """--cell_dir / --nuclei_dir: the decoded label maps of the batch -> per image (cell label map, its largest label, the d2 plane
    or None): DEVICE tensors as cells.CellMap when the run is on the device, host arrays otherwise.  Given cells are taken as they
    are; nuclei become their nearest-nucleus territories, cut at --cell_radius, and bring the squared distance to the nucleus."""
    radius, nuclei, out = run.cells["radius"], run.cells["mode"] == "nuclei", []
    batch.cell_ids = [ids for _, ids in batch.cells]
    for lab, _ in batch.cells:
        top, d2 = max(int(lab.max(initial=0)), 0), None
        if on_device:
            from unet_dc_segmentation_amd.cells import CellMap, nearest_label
            lab = torch.from_numpy(np.ascontiguousarray(lab)).to(DEVICE)
            if nuclei:
                lab, d2 = nearest_label(lab, top, radius)
            out.append(CellMap(lab, top, d2))
        else:
            if nuclei:
                from utils.droplet_cells import nearest_label_numpy
                lab, d2 = nearest_label_numpy(lab, top, radius)
            out.append((lab, top, d2))
    batch.cells = out


def _write_labels16(labels, path):
    from utils.droplet_split import labels_u16
    Image.fromarray(labels_u16(labels)).save(str(path))


def add_cell_outputs(run, df, d, filename, name, cells, ids=None):
    """--cell_dir / --nuclei_dir: the columns of utils.droplet_cells.cell_columns behind the droplet table's own, this image's rows
    of cells.csv and of cells_per_image.csv, with nuclei the territories as a 16-bit label PNG through the writer pool -> (the
    table, the numbers its row of summary_per_image.csv gains).  ids: the file's own cell numbers where decode_cells renumbered them."""
    from utils import droplet_cells as dcell
    rec = d.cells
    if not df.empty:
        df = pd.concat([df, pd.DataFrame(dcell.cell_columns(rec, run.px_per_um, ids), index=df.index)], axis=1)
    run.cells["tables"].append(pd.DataFrame(dcell.cells_table(filename, rec, run.px_per_um, ids)))
    more = dcell.per_image_summary(rec)
    run.cells["rows"].append({"filename": filename, **more})
    if run.cells["dir"] is not None:
        run.submit(_write_labels16, dcell.original_ids(_host(cells[0]), ids), run.cells["dir"] / f"{name}_cells.png")
    return df, more


def add_hull_outputs(run, df, d):
    """--droplet_hull: the columns of utils.droplet_hull.hull_columns behind the droplet table's own -> (the table, the numbers
    its row of summary_per_image.csv gains)."""
    from utils import droplet_hull as dh
    cols = dh.hull_columns(d.hull, d.area, run.hull, run.px_per_um)
    if not df.empty:
        df = pd.concat([df, pd.DataFrame(cols, index=df.index)], axis=1)
    return df, dh.hull_summary(cols)


def outline_records(run, out, on_device):
    """--outlines for one batch: the record of DESIGN.md section 27 per image from the label map of the droplet stage (the split
    one with --split_touching).  On the device the batch is enqueued back to back behind the droplets with one more wait
    (outlines.label_outlines_batch); the rooms come from the areas the table already holds.  Split droplets are basins of the
    watershed and need not be 4-connected: their rooms are the ones of any label."""
    if on_device:
        from unet_dc_segmentation_amd.outlines import label_outlines_batch
        return label_outlines_batch([d.labels for d in out], [d.area for d in out], connected=run.split_depth is None)
    from utils import droplet_outlines as do
    return [do.outlines_numpy(d.labels, len(d.area)) for d in out]


def _write_outlines(rec, path, name, image_id, px_per_um):
    """Writer pool: outlines/NAME.geojson, and the image's COCO annotations for main() to number and write."""
    import json
    from utils import droplet_outlines as do
    with open(path, "w") as f:                           # dumps, not dump: one pass of the C encoder instead of Python chunks
        groups = do.rings(rec)
        f.write(json.dumps(do.geojson(rec, name, px_per_um, groups), separators=(",", ":")))
    return do.coco_annotation(rec, image_id=image_id, groups=groups)


def add_outline_outputs(run, df, d, rec, filename, name, hw):
    """--outlines: the columns of utils.droplet_outlines.outline_columns behind the droplet table's own, the image's GeoJSON file
    and COCO annotations (writer pool) -> (the table, the numbers its row of summary_per_image.csv gains)."""
    from utils import droplet_outlines as do
    cols = do.outline_columns(rec, d.area, run.px_per_um)
    if not df.empty:
        df = pd.concat([df, pd.DataFrame(cols, index=df.index)], axis=1)
    o = run.outlines
    o["images"].append({"id": len(o["images"]) + 1, "file_name": filename, "height": int(hw[0]), "width": int(hw[1])})
    run.submit(_write_outlines, rec, o["dir"] / f"{name}.geojson", name, len(o["images"]), run.px_per_um)
    o["jobs"].append(run.writers[1][-1])
    return df, do.outline_summary(cols)


def add_spatial_outputs(run, batch, out, sums, on_device):
    """--spatial_stats for one batch: the counts of DESIGN.md section 26 from the droplet table alone (on the device from the
    sums the droplet stage left there, one more batch of launches and one more wait; on the CPU from the label map's sums),
    then the rows of spatial_stats.csv and spatial_per_image.csv, which utils.spatial_stats derives on both paths."""
    from utils import spatial_stats as ss
    sp, hws = run.spatial, [m[1] for m in batch.meta]
    windows = batch.windows or [None] * len(hws)
    if on_device:
        from unet_dc_segmentation_amd.spatial import spatial_stats_batch
        wins = [None if win is None else torch.from_numpy(win).to(DEVICE) for win in windows]
        recs = spatial_stats_batch(sums, hws, sp["R"], sp["S"], sp["seed"], wins, masks=[d.mask for d in out])
    else:
        from utils.droplet_match import gt_labels_numpy, label_sums
        recs = []
        for d, hw, win in zip(out, hws, windows):
            lab = d.labels if d.labels is not None else gt_labels_numpy(d.mask, run.min_area)
            recs.append(ss.spatial_record(*label_sums(lab), *hw, sp["R"], sp["S"], sp["seed"], win))
    for rec, (fpath, _) in zip(recs, batch.meta):
        filename = Path(fpath).name
        res = ss.analyse(rec["n"], rec["pairs"], rec["pairs_all"], rec["A"], rec["N"])
        sp["rows"].append(ss.summary_row(filename, rec, res))
        sp["table"].extend(ss.table_rows(filename, (rec["n"], rec["pairs"], rec["pairs_all"]), res, run.px_per_um))


def _write_map(plane, path):
    Image.fromarray(plane).save(str(path))


def _write_picture(rgb, path):
    """A full-size RGB PNG of --diff_maps.  zlib level 1: on a 1040 x 1388 overlay PIL's default level 6 takes 3.4 times as
    long for a file 5 % smaller, and the two pictures are most of what the flag costs per image."""
    Image.fromarray(rgb).save(str(path), compress_level=1)


def add_diff_outputs(run, batch, out):
    """--diff_maps for one batch: the difference map of every measured mask (after cleaning, at the image's size) against its
    annotation (> 0, labels included), the overlay on the decoded image, this image's rows of diff_regions.csv and its row of
    diff_regions_per_image.csv.  On the device the batch is enqueued back to back with one host wait
    (evaluate.diff_regions_batch) and reads the images already uploaded; the PNGs go through the writer pool."""
    from utils import difference_map as dmap
    diff = run.diff
    gts = [np.ascontiguousarray(np.asarray(_host(g)) > 0, dtype=np.uint8) for g in batch.gt_items]
    if torch.is_tensor(out[0].mask) and out[0].mask.is_cuda:
        from unet_dc_segmentation_amd.evaluate import diff_regions_batch
        recs = diff_regions_batch([d.mask.contiguous() for d in out], [torch.from_numpy(g).to(DEVICE) for g in gts],
                                  diff["min_area"], batch.rgbs, paint=True)
    else:
        recs = []
        for d, g, rgb in zip(out, gts, batch.rgbs):
            mask = _host(d.mask)
            recs.append({**dmap.diff_regions_numpy(mask, g, diff["min_area"]), "diff": dmap.difference_map_rgb(mask, g),
                         "overlay": dmap.overlay_difference(_host(rgb), mask, g)})
    for rec, (fpath, _) in zip(recs, batch.meta):
        filename, name = Path(fpath).name, Path(fpath).stem
        diff["tables"].append(pd.DataFrame(dmap.region_table(filename, rec, run.px_per_um)))
        diff["rows"].append({"filename": filename, **dmap.image_columns(rec)})
        run.submit(_write_picture, _host(rec["diff"]), diff["map_dir"] / f"{name}_diffmap.png")
        run.submit(_write_picture, _host(rec["overlay"]), diff["overlay_dir"] / f"{name}_overlay.png")


def quantify(bin_mask, min_area, px_per_um, split_depth=None):
    """Per-droplet table: label, area, equivalent_diameter, centroid-0/1 (+ micron columns) -- CPU path (SciPy).
    split_depth (pixels): the table of the split droplets instead (utils/droplet_split.py)."""
    _, area, cy, cx = droplets_cpu(bin_mask, min_area, split_depth)
    return _droplet_table(area, cy, cx, px_per_um)


def quantify_device(probs2d, thresh, out_hw, min_area, px_per_um):
    """The same table from the probability map still on the HIP device; also returns the uint8 mask (host) for the PNG."""
    from unet_dc_segmentation_amd.droplets import mask_and_droplets
    d = mask_and_droplets(probs2d, thresh, out_hw, min_area)
    return d.mask.cpu().numpy(), _droplet_table(d.area, d.centroid_row, d.centroid_col, px_per_um)


def _outline(mask):
    from scipy import ndimage
    return mask.astype(bool) & ~ndimage.binary_erosion(mask.astype(bool), iterations=2)


def _write_outputs(mask, df, fpath, name, mask_dir, overlay_dir, labels=None, img=None):
    """The per-image files of run_batch (reference :66-79): mask PNG, droplet CSV, optional overlay; with --split_touching
    (labels given) the 16-bit label image as well, and the overlay's outline follows the cuts.  img: the windowed 8-bit image
    of a run with a window flag, which the overlay is painted on in place of the file's clipped pixels."""
    Image.fromarray(mask * 255).save(str(mask_dir / f"{name}_pred.png"))
    df.to_csv(mask_dir.parent / f"{name}_droplets.csv", index=False)
    if labels is not None:
        from utils.droplet_split import labels_u16
        Image.fromarray(labels_u16(labels)).save(str(mask_dir / f"{name}_labels.png"))
    if overlay_dir is not None:
        img = np.array(Image.open(fpath).convert("RGB")) if img is None else np.array(img)
        img[_outline(mask)] = (0, 255, 0)
        if labels is not None:
            from utils.droplet_split import label_boundaries
            img[label_boundaries(labels)] = (0, 255, 0)
        Image.fromarray(img).save(str(overlay_dir / f"{name}_overlay.png"))


def _density(run, dres, rgb, mask, fpath):
    """--density_maps for one image: the row of density_per_image.csv, and the two heat-map PNGs (colormap gather and deflate
    in the writer pool).  dres: the device results of the batch for this image, or None on the CPU path."""
    from utils import density as hd
    nb_layers = run.density["nb_layers"]
    r = hd.density_maps(rgb, mask, nb_layers, run.density["kernel"]) if dres is None else dres
    run.density_rows.append(hd.csv_row(Path(fpath).name, r, nb_layers))
    run.submit(hd.write_pngs, r["radial_index"], r["spatial_index"], run.out_dir, Path(fpath).stem)


def _cpu_mask(p2, thresh, hw, clean):
    """CPU path: probabilities [h, w] (numpy fp32) -> (the mask every stage sees at one threshold: resize, then the cleaning
    options of the run; the int64 [4] counts of the cleaning, zeros without)."""
    oh, ow = hw
    mask = resize_mask_like_reference((p2 > np.float32(thresh)).astype(np.uint8), ow, oh)
    if clean is None:
        return mask, np.zeros(4, np.int64)
    from utils.droplet_clean import clean_mask
    weak = None                                          # both masks under the same resize rule
    if clean["low"] is not None:
        weak = resize_mask_like_reference((p2 > np.float32(clean["low"])).astype(np.uint8), ow, oh)
    return clean_mask(mask, weak, clean["holes"])


def droplets_and_matches(run, batch, probs, thresh, sweeping=False, envelope=None):
    """The droplet stage at one threshold, and with --gt_dir the matching of its label maps against the batch's annotations
    -> (one Droplets per image, one match result per image or None, the density stage's device sums or None).  On the
    device the whole batch is enqueued back to back with ONE host wait (droplets.py), and one more for the matching; on the
    CPU the same records come from droplets_cpu and match_cpu.  sweeping: a threshold of --sweep_objects, where only the
    matching is read: no shape columns, no grey planes, no boundary distances.  With --boundary every match result carries the
    record of DESIGN.md section 21 under "boundary" (device: one more batch of launches and one more wait, evaluate.boundary_batch).
    With --droplet_hull (never while sweeping) every Droplets carries the integers of DESIGN.md section 24.
    With --outlines (never while sweeping) every Droplets carries its label map, which finish_batch hands to the outline stage.
    With --confidence (never while sweeping) every Droplets carries the record of DESIGN.md section 23; envelope: the (lo, hi) maps
    of --tta, shaped like probs.  With --cell_dir / --nuclei_dir (never while sweeping) every Droplets carries the record of DESIGN.md
    section 31 against batch.cells, which cell_maps has prepared."""
    gt, hws = run.gt, [m[1] for m in batch.meta]
    radius = run.boundary["R"] if run.boundary is not None and not sweeping else None
    want_labels = gt is not None or run.split_depth is not None or (run.outlines is not None and not sweeping)
    shape = run.shape and not sweeping
    conf = run.confidence if not sweeping else None
    hull = run.hull is not None and not sweeping
    cells = batch.cells if run.cells is not None and not sweeping else None
    if probs.is_cuda:
        from unet_dc_segmentation_amd.droplets import mask_and_droplets_batch
        gray = [torch.from_numpy(g).to(DEVICE) for g in batch.grays] if shape else None   # up behind the network's launches
        more = {} if conf is None or envelope is None else {"envelope": tuple(e[:, 0] for e in envelope)}
        if cells is not None:
            more["cells"] = cells
        out, sums = mask_and_droplets_batch(probs[:, 0], thresh, hws, run.min_area, keep_sums=True, gray=gray,
                                            options=run.droplet_options(want_labels, shape, conf is not None, hull, cells is not None), **more)
        if gt is None:
            return out, None, sums
        from unet_dc_segmentation_amd.evaluate import boundary_batch, match_batch
        labs, areas = [d.labels for d in out], [d.area for d in out]
        if radius is None:
            return out, match_batch(labs, areas, batch.gt_items, gt["min_area"], gt["labels"]), sums
        mres = match_batch(labs, areas, batch.gt_items, gt["min_area"], gt["labels"], keep_labels=True)
        recs = boundary_batch(labs, [len(a) for a in areas], [r.pop("gt_labels") for r in mres], [len(r["gt_area"]) for r in mres],
                              radius)
        for r, rec in zip(mres, recs):
            r["boundary"] = rec
        return out, mres, sums
    out, p = [], probs[:, 0].numpy()
    for i, hw in enumerate(hws):
        mask, counts = _cpu_mask(p[i], thresh, hw, run.clean)
        ckw = None
        if conf is not None:
            lo, hi = (None, None) if envelope is None else (e[i, 0].numpy() for e in envelope)
            ckw = {"probs": p[i], "thresh": thresh, "band": conf["band"], "lo": lo, "hi": hi, "maps": conf["maps"]}
        d = droplets_cpu(mask, run.min_area, run.split_depth, shape, batch.grays[i] if shape else None, want_labels, run.neighbors, ckw, hull,
                         None if cells is None else cells[i])
        d.clean_counts = np.asarray(counts, np.int64)
        out.append(d)
    if gt is None:
        return out, None, None
    return out, [match_cpu(d.labels, d.area, item, gt["min_area"], gt["labels"], radius) for d, item in zip(out, batch.gt_items)], None


def sweep_step(run, batch, probs):
    """--thresh_sweep for one batch: the batch's probabilities against its annotations at every threshold of the grid, added
    into the run's histogram (on the device: unetdc_thresh_sweep, nothing waits; on the CPU: sweep_hist_numpy).  Then, for
    every threshold of --sweep_objects, the droplet stage with the run's own split / clean options and the matching of
    --gt_dir once more on the same probabilities: the integers of one match_per_image.csv row per image and threshold."""
    sweep, hws = run.sweep, [m[1] for m in batch.meta]
    if probs.is_cuda:
        from unet_dc_segmentation_amd.evaluate import sweep_batch
        sweep["hist"] = sweep_batch(probs[:, 0], batch.gt_items, hws, sweep["K"], hist=sweep["hist"])
    else:
        from utils.threshold_sweep import sweep_hist_numpy
        for p2, item, hw in zip(probs[:, 0].numpy(), batch.gt_items, hws):
            h = sweep_hist_numpy(p2, item, hw, sweep["K"])
            sweep["hist"] = h if sweep["hist"] is None else sweep["hist"] + h
    for t in sweep["objects"]:
        res = droplets_and_matches(run, batch, probs, t, sweeping=True)[1]
        sweep["object_images"][t].extend(r["columns"]["image"] for r in res)


@torch.no_grad()
def run_batch(run, batch, model):
    x = torch.stack(batch.tensors).to(DEVICE)
    more = {"envelope": True} if run.envelope else {}    # --tta with --confidence: (mean, lo, hi) from the same launch
    if run.tta is None:
        probs = model(x)                                 # sigmoid probabilities (model_2.py:80)
    elif x.is_cuda:                                      # --tta: the mean over the variants, tta["batch"] items per forward
        from unet_dc_segmentation_amd.tta import predict_tta
        probs = predict_tta(model, x, run.tta["N"], run.tta["batch"], **more)
    else:
        from utils.tta import predict_tta_cpu
        probs = predict_tta_cpu(model, x, run.tta["N"], run.tta["batch"], **more)
    finish_batch(run, batch, probs)


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def finish_batch(run, batch, probs):
    """Everything behind the forward: probs [B, 1, ph, pw] (on the device or not) -> masks of the sizes in batch.meta, droplet
    tables, the optional stages and the per-image files.  run_batch feeds it the network-size maps, --tile one native-size map
    per image (ph, pw equal to the image's size: every resize rule is then the identity).  probs may be the triple (mean, lo,
    hi) of --tta with --confidence: every stage reads the mean, the confidence stage the envelope as well."""
    envelope = None
    if isinstance(probs, tuple):
        probs, envelope = probs[0], probs[1:]
    if run.gt is not None and run.gt.get("polygons") is not None:
        rasterize_gt(run, batch, probs.is_cuda)           # --gt_polygons: label maps from here on, as --gt_labels decodes them
    if run.cells is not None:
        cell_maps(run, batch, probs.is_cuda)              # --nuclei_dir: the territories, ahead of the droplet stage on its stream
    if run.sweep is not None:                           # --thresh_sweep: the raw mask at every threshold, pooled
        sweep_step(run, batch, probs)
    out, mres, sums = droplets_and_matches(run, batch, probs, run.thresh, envelope=envelope)
    dres = None
    if run.density is not None and probs.is_cuda:
        from unet_dc_segmentation_amd.density import density_maps_batch
        # the maps count every connected component: the table's sums serve when min_area <= 1 and no option changed the stage
        plain = run.split_depth is None and not run.shape and run.gt is None and run.clean is None
        dres = density_maps_batch(batch.rgbs, [d.mask for d in out], sums if run.min_area <= 1 and plain else None,
                                  run.density["nb_layers"], run.density["kernel"])
    if run.diff is not None:
        add_diff_outputs(run, batch, out)
    if run.spatial is not None:
        add_spatial_outputs(run, batch, out, sums, probs.is_cuda)
    orecs = outline_records(run, out, probs.is_cuda) if run.outlines is not None else None
    for i, (d, (fpath, hw)) in enumerate(zip(out, batch.meta)):
        filename, name = Path(fpath).name, Path(fpath).stem
        mask = _host(d.mask)
        labels = _host(d.labels) if run.split_depth is not None else None       # --split_touching writes them
        df = _droplet_table(d.area, d.centroid_row, d.centroid_col, run.px_per_um)
        if run.shape:
            df = add_shape_columns(df, d.props, hw, run.px_per_um)
        if mres is not None:
            df = add_match_outputs(run, df, mres[i], filename)
        more = {}
        if run.neighbors is not None:
            df, more = add_neighbor_outputs(run, df, d, filename)
        if run.confidence is not None:
            df = add_confidence_outputs(run, df, d, filename, name)
        if run.hull is not None:
            df, hull_more = add_hull_outputs(run, df, d)
            more = {**more, **hull_more}
        if orecs is not None:
            df, outline_more = add_outline_outputs(run, df, d, orecs[i], filename, name, hw)
            more = {**more, **outline_more}
        if run.cells is not None:
            df, cell_more = add_cell_outputs(run, df, d, filename, name, batch.cells[i], batch.cell_ids[i])
            more = {**more, **cell_more}
        if run.clean is not None:
            from utils.droplet_clean import COUNT_NAMES
            run.clean["rows"].append({"filename": filename, **{k: int(v) for k, v in zip(COUNT_NAMES, d.clean_counts)}})
        df.insert(0, "filename", filename) if not df.empty else None
        run.tables.append(df)
        run.rows.append({"filename": filename, "droplet_count": len(df), "total_area_px": df["area"].sum() if not df.empty else 0, **more})
        windowed = _host(batch.rgbs[i]) if run.intensity is not None and run.overlay_dir is not None else None
        run.submit(_write_outputs, mask, df, fpath, name, run.mask_dir, run.overlay_dir, labels, windowed)
        if run.density is not None:
            _density(run, None if dres is None else dres[i], batch.rgbs[i], mask, fpath)
        # back-pressure: at most ~4 batches of masks / tables wait for the writers; waiting on the OLDEST write also surfaces a
        # failed write while the run is still going
        while len(run.writers[1]) > run.writers[2]:
            run.writers[1].popleft().result()


def _radius_arg(text):
    from utils.droplet_neighbors import check_radius
    try:
        return check_radius(int(text))
    except ValueError:
        raise argparse.ArgumentTypeError(f"G must be an integer number of pixels in 1..64, not {text!r}")


def _spatial_radius_arg(text):
    from utils.spatial_stats import check_radius
    try:
        return check_radius(int(text))
    except ValueError:
        raise argparse.ArgumentTypeError(f"R must be an integer number of pixels in 1..256, not {text!r}")


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
    p.add_argument("--gt_polygons", metavar="PATH",
                   help="score against polygon annotations instead of --gt_dir: a directory with NAME.geojson per image (as "
                        "--outlines writes them), or a COCO .json file whose images are matched by the stem of file_name.  The "
                        "polygons are filled by the exact rule of DESIGN.md section 28 (on the device where the run is) and "
                        "behave as --gt_dir with --gt_labels from then on; --gt_min_area does not apply")
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
    p.add_argument("--neighbors", type=_radius_arg, nargs="?", const=5, metavar="G",
                   help="droplet neighbourhoods: two droplets are in contact when their closest pixels are at most G pixels "
                        "apart (pixel centres, Euclidean; G in 1..64, 5 without G -- a convention, not a measured number); adds "
                        "nn_label, nn_dist_px, nn_centroid_dist_px, n_contacts, cluster, cluster_size (and nn_dist_micron with "
                        "--px_per_micron) to the droplet tables, contact and cluster counts to summary_per_image.csv, and writes "
                        "droplet_contacts.csv (filename, label_a, label_b, d2, dist_px).  With --split_touching the cut droplets "
                        "touch (d2 = 1); components below --min_area are background")
    p.add_argument("--boundary", type=int, nargs="?", const=64, metavar="R",
                   help="with --gt_dir: boundary accuracy against the annotation -- for every boundary pixel of the predicted "
                        "label map (the cuts of --split_touching and the image frame included) the distance to the nearest "
                        "boundary pixel of the annotated one, and back; distances beyond R pixels (1..64, 64 without R) count as "
                        "far.  Adds bd_px, bd_rms, bd_max to the droplet tables and to gt_droplets.csv (distances to the nearest "
                        "boundary of ANY object of the other map, not of the matched partner) and writes boundary_per_image.csv: "
                        "Hausdorff distance, HD95, average symmetric surface distance, and per tolerance boundary precision, "
                        "recall, F and surface Dice (nsd), one row per image and the pooled row ALL")
    p.add_argument("--boundary_tol", metavar="T[,T...]",
                   help="with --boundary: the integer pixel tolerances of the surface Dice columns (0..R, default 1,2,3)")
    p.add_argument("--confidence", type=float, nargs="?", const=0.1, metavar="BAND",
                   help="per-droplet confidence: adds prob_mean, prob_std, prob_min, prob_max, entropy_mean (bits) and "
                        "uncertain_frac (pixels whose probability lies within BAND of --prob_thresh; BAND in 0..0.5, 0.1 without "
                        "BAND -- a convention, not a measured number) to the droplet tables, and with --tta the disagreement of "
                        "the variants: tta_spread_mean, tta_spread_max, unstable_frac (pixels some variants put above the "
                        "threshold and some not).  Writes confidence_per_image.csv: mean entropy over the image and over its "
                        "background, uncertain pixels in all and on the background (the missed-droplet indicator), unstable pixels, "
                        "mean spread, droplets and their lowest prob_mean -- which images to look at, or annotate, next.  "
                        "Probabilities are read at the nearest source pixel of each mask pixel and quantised to 16 bits")
    p.add_argument("--confidence_maps", action="store_true",
                   help="with --confidence: also write NAME_entropy.png and, with --tta, NAME_spread.png (8-bit maps)")
    p.add_argument("--droplet_hull", type=float, nargs="?", const=0.9, metavar="S",
                   help="per-droplet convex hull of the pixel squares: adds area_convex, solidity (area / area_convex: a single "
                        "droplet is convex and near 1, two fused ones are not), feret_diameter_max and feret_diameter_min (the "
                        "largest and smallest caliper width), feret_ratio, hull_vertices and low_solidity (solidity < S; S in "
                        "(0, 1], 0.9 without S -- a convention, not a measured number) to the droplet tables, with "
                        "--px_per_micron also feret_max_micron, feret_min_micron, area_convex_sqmicron; summary_per_image.csv "
                        "gains solidity_median, feret_max_median and n_low_solidity")
    p.add_argument("--diff_maps", type=int, nargs="?", const=1, metavar="MIN_AREA",
                   help="with --gt_dir: where the prediction fails -- writes difference_maps/NAME_diffmap.png (yellow: predicted "
                        "and annotated, red: only annotated, green: only predicted, black: neither) and "
                        "diff_overlays/NAME_overlay.png (that map over the original image), diff_regions.csv (one row per "
                        "8-connected red, green or yellow region of at least MIN_AREA pixels, 1 without MIN_AREA: class, area, "
                        "centroid, touches_common = it borders a yellow region, isolated = a red or green one that does not: a "
                        "droplet missed entirely, or a spurious one) and diff_regions_per_image.csv (yellow / red / green / black "
                        "regions = region-level TP / FN / FP / TN, their pixels, the regions kept, missed_droplets, "
                        "spurious_droplets).  The prediction is the mask the droplet stage measured (after --prob_thresh_low / "
                        "--fill_holes), the annotation is grey > 0, with --gt_labels label > 0; --gt_min_area does not apply here")
    iw.add_flags(p)
    p.add_argument("--outlines", action="store_true",
                   help="per-droplet outlines as polygons (crack-following contours of the label map, holes as inner rings): adds "
                        "perimeter_crack (boundary length in pixel edges, a city-block length), n_holes, euler_number, area_filled, "
                        "hole_area and outline_vertices to the droplet tables, n_with_holes and hole_area_total to "
                        "summary_per_image.csv, and writes outlines/NAME.geojson per image and one outlines_coco.json (outer rings "
                        "only) for annotation tools; with --split_touching the outlines follow the cuts")
    p.add_argument("--spatial_stats", type=_spatial_radius_arg, nargs="?", const=64, metavar="R",
                   help="Ripley's K(r), L(r) - r and g(r) of the droplet centroids for r = 1..R pixels (default 64, at most 256), "
                        "border-corrected, with the envelope of --spatial_sims patterns of complete spatial randomness in the "
                        "same window: spatial_stats.csv (one row per image and r) and spatial_per_image.csv (csr_p, pattern)")
    p.add_argument("--spatial_sims", type=int, default=99, metavar="S",
                   help="simulated patterns behind the envelope and csr_p of --spatial_stats, 0..999 (0: no envelope)")
    p.add_argument("--spatial_seed", type=int, default=0, help="32-bit seed of the simulated patterns of --spatial_stats")
    p.add_argument("--spatial_window_dir", metavar="D",
                   help="observation windows of --spatial_stats: the window of NAME.ext is D/NAME.<image suffix>, nonzero = "
                        "inside, of its image's size; without it the window is the whole image")
    p.add_argument("--cell_dir", metavar="C",
                   help="droplets per cell, the cells given: the mask of NAME.ext is C/NAME.<image suffix> (the rule of --gt_dir), a "
                        "binary mask whose 4-connected components of at least --cell_min_area pixels are the cells, or with "
                        "--cell_labels a label image.  Adds cell, cell_overlap_frac, n_cells, outside_cells to the droplet tables, "
                        "writes cells.csv and cells_per_image.csv and adds the latter's columns to summary_per_image.csv")
    p.add_argument("--nuclei_dir", metavar="N",
                   help="droplets per cell, the nuclei given (read like --cell_dir): the cells are the territories of the nearest "
                        "nucleus, cut at --cell_radius; also nucleus_gap_px per droplet, nucleus_area_px per cell and "
                        "cell_territories/NAME_cells.png (16-bit labels)")
    p.add_argument("--cell_radius", type=int, metavar="R",
                   help="with --nuclei_dir: pixels further than R from every nucleus belong to no cell (default 0: unbounded)")
    p.add_argument("--cell_min_area", type=int, default=1, help="ignore cells / nuclei of a binary mask smaller than this (pixels^2)")
    p.add_argument("--cell_labels", action="store_true",
                   help="the files of --cell_dir / --nuclei_dir are label images (16-bit, or any integer image), taken as they are")
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
    if not (args.gt_dir or args.gt_polygons):
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


def boundary_options(args):
    """--boundary / --boundary_tol -> {"R", "tols", "records"}, None without the flag; a bad value or a missing --gt_dir ends
    the run before any image."""
    if args.boundary is None:
        if args.boundary_tol is not None:
            raise SystemExit("--boundary_tol needs --boundary")
        return None
    if not (args.gt_dir or args.gt_polygons):
        raise SystemExit("--boundary measures against annotated masks: it needs --gt_dir")
    from utils.droplet_boundary import DEFAULT_TOLS, check_radius, check_tols
    try:
        R = check_radius(args.boundary)
        tols = DEFAULT_TOLS if args.boundary_tol is None else [int(v) for v in args.boundary_tol.split(",") if v.strip()]
        tols = check_tols([t for t in tols if args.boundary_tol is not None or t <= R], R)
    except ValueError as e:
        raise SystemExit(f"--boundary R / --boundary_tol: {e}")
    return {"R": R, "tols": tols, "records": []}


def confidence_options(args):
    """--confidence / --confidence_maps -> {"band", "maps", "rows"}, None without the flag; a bad value ends the run before any
    image."""
    if args.confidence is None:
        if args.confidence_maps:
            raise SystemExit("--confidence_maps needs --confidence")
        return None
    from utils.droplet_confidence import check_band
    try:
        band = check_band(args.confidence)
    except ValueError as e:
        raise SystemExit(f"--confidence BAND: {e}")
    return {"band": band, "maps": bool(args.confidence_maps), "rows": []}


def spatial_options(args, images):
    """--spatial_stats -> {"R", "S", "seed", "files" ({image path: window path} or None), "table", "rows"} or None; every window
    is there and of its image's size, or nothing runs."""
    if args.spatial_stats is None:
        if args.spatial_window_dir:
            raise SystemExit("--spatial_window_dir belongs to --spatial_stats")
        return None
    from utils.spatial_stats import check_sims
    try:
        sims = check_sims(args.spatial_sims)
    except ValueError as e:
        raise SystemExit(f"--spatial_sims S: {e}")
    if not 0 <= args.spatial_seed < 2 ** 32:
        raise SystemExit("--spatial_seed must be in 0..2^32 - 1")
    files = None
    if args.spatial_window_dir:
        files = find_gt_files(images, args.spatial_window_dir, "--spatial_window_dir", "window")
    return {"R": args.spatial_stats, "S": sims, "seed": args.spatial_seed, "files": files, "table": [], "rows": []}


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
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.gt_dir and args.gt_polygons:
        parser.error("--gt_polygons and --gt_dir are two sources of the same annotation: give one")
    if args.diff_maps is not None and not (args.gt_dir or args.gt_polygons):
        parser.error("--diff_maps compares against annotated masks: it needs --gt_dir")
    if args.diff_maps is not None and args.diff_maps < 1:
        parser.error("--diff_maps MIN_AREA: MIN_AREA is a number of pixels, at least 1")
    from utils import droplet_cells as dcell
    try:
        cell_mode = dcell.check_flags(args.cell_dir, args.nuclei_dir, args.cell_radius, args.cell_labels)
    except ValueError as e:
        parser.error(str(e))
    in_dir, out_dir = Path(args.img_dir), Path(args.out_dir)
    try:                                                 # checked before any image, and before any output directory exists
        spec = iw.spec_from_flags(args.intensity_window, args.intensity_levels, args.page)
    except ValueError as e:
        parser.error(str(e))
    intensity = None if spec is None else {"spec": spec, "records": []}
    iw.clip_warner.done = False
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
    boundary = boundary_options(args)
    confidence = confidence_options(args)
    hull = None
    if args.droplet_hull is not None:
        from utils.droplet_hull import check_solidity
        try:
            hull = check_solidity(args.droplet_hull)
        except ValueError as e:
            raise SystemExit(f"--droplet_hull S: {e}")
    images = sorted(p for p in in_dir.iterdir() if p.suffix.lower() in IMAGE_SUFFIXES)
    gt = None
    if args.gt_dir:                                      # every annotation is there and of its image's size, or nothing runs
        gt = {"files": find_gt_files(images, args.gt_dir), "min_area": args.gt_min_area, "labels": args.gt_labels}
    elif args.gt_polygons:                               # every polygon file is there (COCO: read, and of its image's size), or nothing runs
        gt = {"polygons": find_gt_polygons(images, args.gt_polygons), "min_area": 1, "labels": True, "features": 0, "dropped": 0}
    cells = None
    if cell_mode is not None:                            # every mask is there and of its image's size, or nothing runs
        flag = "--cell_dir" if cell_mode == "cells" else "--nuclei_dir"
        cells = {"mode": cell_mode, "files": find_gt_files(images, args.cell_dir or args.nuclei_dir, flag, "cell mask" if cell_mode == "cells" else "nuclei mask"),
                 "labels": args.cell_labels, "min_area": args.cell_min_area, "radius": args.cell_radius or 0,
                 "dir": out_dir / "cell_territories" if cell_mode == "nuclei" else None, "tables": [], "rows": []}
    spatial = spatial_options(args, images)
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
        density = {"nb_layers": args.nb_layers, "kernel": args.density_kernel}
    diff = None
    if args.diff_maps is not None:
        diff = {"min_area": args.diff_maps, "map_dir": out_dir / "difference_maps", "overlay_dir": out_dir / "diff_overlays",
                "tables": [], "rows": []}
        diff["map_dir"].mkdir(exist_ok=True)
        diff["overlay_dir"].mkdir(exist_ok=True)
    outlines = None
    if args.outlines:
        outlines = {"dir": out_dir / "outlines", "images": [], "jobs": []}
        outlines["dir"].mkdir(exist_ok=True)
    if cells is not None and cells["dir"] is not None:
        cells["dir"].mkdir(exist_ok=True)
    model = load_model(args.ckpt_path, args.dtype)
    # File decode runs ahead of the device and the per-image writes behind it, in two small thread pools (both are
    # zlib-bound and release the GIL); the order of the rows in the summary files is the order of `images` as before.
    import os
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    nthreads = max(1, min(8, (os.cpu_count() or 2) // 2))
    with ThreadPoolExecutor(nthreads) as dec_pool, ThreadPoolExecutor(nthreads) as wr_pool:
        run = Run(thresh=args.prob_thresh, min_area=args.min_area, px_per_um=args.px_per_micron,
                  background_radius=args.background_radius, batch_size=args.batch, split_depth=split_depth,
                  shape=args.droplet_shape, clean=clean, sweep=sweep, tile=tile, tta=tta, density=density, gt=gt, out_dir=out_dir,
                  mask_dir=mask_dir, overlay_dir=overlay_dir, writers=(wr_pool, deque(), 4 * max(1, args.batch)),
                  neighbors=args.neighbors, boundary=boundary, confidence=confidence, hull=hull, diff=diff,
                  spatial=spatial, outlines=outlines, intensity=intensity, cells=cells)
        ahead = deque()
        it = iter(images)

        def refill():
            while len(ahead) < 2 * args.batch:
                nxt = next(it, None)
                if nxt is None:
                    return
                ahead.append((nxt, dec_pool.submit(decode_image, nxt, intensity),
                              None if gt is None else dec_pool.submit(decode_gt_polygons, gt["polygons"][str(nxt)]) if "polygons" in gt
                              else dec_pool.submit(decode_gt, gt["files"][str(nxt)], gt["labels"]),
                              None if spatial is None or spatial["files"] is None
                              else dec_pool.submit(decode_gt, spatial["files"][str(nxt)], False),
                              None if cells is None else dec_pool.submit(decode_cells, cells["files"][str(nxt)], cells["labels"], cells["min_area"])))

        refill()
        batch = Batch()
        while ahead:
            img, fut, gt_fut, win_fut, cell_fut = ahead.popleft()
            refill()
            im = fut.result()
            if intensity is not None:                    # the windowed 8-bit image stands for the original from here on
                im = window_image(run, img, *im)
            batch.meta.append((str(img), tuple(int(v) for v in im.shape[:2])))
            if run.shape:                                # the ORIGINAL image as grey, before the rolling ball
                from utils.density import rgb_to_gray
                batch.grays.append(rgb_to_gray(_host(im)))
            if gt is not None:
                batch.gt_items.append(gt_fut.result())
            if win_fut is not None:
                batch.windows.append(win_fut.result())
            if cell_fut is not None:
                batch.cells.append(cell_fut.result())
            if tile is not None:                         # native size: one map per image, the stages on a batch of one
                probs, rgb = predict_tiled_image(model, _host(im), run)
                batch.rgbs.append(rgb)
                finish_batch(run, batch, probs)
                batch = Batch()
                continue
            t, _, *rgb = preprocess(img, args.background_radius, im, keep_rgb=run.keep_rgb)
            batch.tensors.append(t)
            batch.rgbs += rgb
            if len(batch.tensors) == args.batch:
                run_batch(run, batch, model)
                batch = Batch()
        if batch.tensors:
            run_batch(run, batch, model)
        for f in run.writers[1]:
            f.result()                                   # re-raises a failed write
    if intensity is not None:
        rows = [iw.record_row(name, mode, spec, n, {k: _host(v) for k, v in rec.items()}) for name, mode, n, rec in intensity["records"]]
        pd.DataFrame(rows).to_csv(out_dir / "intensity_per_image.csv", index=False)
    if density is not None:
        pd.DataFrame(run.density_rows).to_csv(out_dir / "density_per_image.csv", index=False)
    if gt is not None:
        from utils.droplet_match import pooled_row, summary_row
        tables = [t for t in run.gt_tables if len(t)] or run.gt_tables[:1]
        pd.concat(tables, ignore_index=True).to_csv(out_dir / "gt_droplets.csv", index=False) if tables else None
        rows = [summary_row(name, ints) for name, ints in run.gt_images] + [pooled_row([ints for _, ints in run.gt_images])]
        pd.DataFrame(rows).to_csv(out_dir / "match_per_image.csv", index=False)
        if "polygons" in gt:
            print(f"--gt_polygons: {gt['dropped']} of {gt['features']} features own no pixel centre and were dropped")
    if boundary is not None:
        from utils import droplet_boundary as db
        recs = boundary["records"]
        rows = [db.summary_row(name, h, d, boundary["R"], boundary["tols"]) for name, h, d in recs]
        rows.append(db.pooled_row([(h, d) for _, h, d in recs], boundary["R"], boundary["tols"]))
        pd.DataFrame(rows, columns=db.column_names(boundary["tols"])).to_csv(out_dir / "boundary_per_image.csv", index=False)
    if confidence is not None:
        from utils.droplet_confidence import IMAGE_COLUMNS
        pd.DataFrame(confidence["rows"], columns=("filename",) + IMAGE_COLUMNS).to_csv(out_dir / "confidence_per_image.csv", index=False)
    if diff is not None:
        from utils import difference_map as dmap
        tables = [t for t in diff["tables"] if len(t)] or diff["tables"][:1]
        pd.concat(tables, ignore_index=True).to_csv(out_dir / "diff_regions.csv", index=False) if tables else None
        pd.DataFrame(diff["rows"], columns=("filename",) + dmap.IMAGE_COLUMNS).to_csv(out_dir / "diff_regions_per_image.csv", index=False)
    if spatial is not None:
        from utils import spatial_stats as ss
        pd.DataFrame(spatial["table"], columns=ss.table_columns(run.px_per_um)).to_csv(out_dir / "spatial_stats.csv", index=False)
        pd.DataFrame(spatial["rows"], columns=ss.IMAGE_COLUMNS).to_csv(out_dir / "spatial_per_image.csv", index=False)
    if cells is not None:
        tables = [t for t in cells["tables"] if len(t)] or cells["tables"][:1]
        if tables:
            pd.concat(tables, ignore_index=True).to_csv(out_dir / "cells.csv", index=False)
        pd.DataFrame(cells["rows"], columns=("filename",) + dcell.SUMMARY_NAMES).to_csv(out_dir / "cells_per_image.csv", index=False)
    if outlines is not None:                             # one COCO file for the run: annotation ids count through the images
        import json
        anns = [a for job in outlines["jobs"] for a in job.result()]
        for i, a in enumerate(anns, start=1):
            a["id"] = i
        with open(out_dir / "outlines_coco.json", "w") as f:
            f.write(json.dumps({"images": outlines["images"], "annotations": anns, "categories": [{"id": 1, "name": "droplet"}]},
                               separators=(",", ":")))
    if clean is not None:
        pd.DataFrame(clean["rows"]).to_csv(out_dir / "mask_clean_per_image.csv", index=False)
    if run.neighbors is not None and run.contact_tables:
        pd.concat(run.contact_tables, ignore_index=True).to_csv(out_dir / "droplet_contacts.csv", index=False)
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
    summary_df = pd.DataFrame(run.rows)
    summary_df.to_csv(out_dir / "summary_per_image.csv", index=False)
    props = [d for d in run.tables if not d.empty]
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
