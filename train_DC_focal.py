#!/usr/bin/env python3
"""Training entry point -- drop-in for the reference's ``train_DC_focal.py`` on the MI355X path.

The reference is a module-level script with hard-coded constants; this keeps its loop
(train_DC_focal.py:241-358: Adam lr 1e-3, 15 epochs, batch 8, focal+dice (1.0, 2.0, 0.3),
0.3 threshold metrics, early stopping on validation Dice with patience 5, best ``state_dict`` saved
to ``best_UNetDC_focal_model.pth``) behind argparse flags whose defaults are those constants.
New: ``--synthetic`` (seeded droplet tiles, no dataset needed), ``--dtype`` (f32 | bf16 compute on
the HIP path), ``--steps`` (cap the steps per epoch), and data-parallel training when launched with
``python -m torch.distributed.run --nproc-per-node N train_DC_focal.py ...`` (RCCL all-reduce
overlapped with backward, unet_dc_segmentation_amd/dp.py), and ``--device_data`` (images preprocessed once into a cache on the
device, each batch augmented there: unet_dc_segmentation_amd/device_data.py; with ``--crop S`` the cache keeps the images at
their own size and every batch is S x S random windows).  The numbers of the reference's test section (:365-402, :452-467:
best checkpoint reloaded, test loss / Dice / pixel accuracy, precision / recall / F1 / specificity / confusion matrix) are
computed and printed (with ``--tta N`` on the network's mean over N flipped and rotated variants of every input, as is
``--calibrate_thresh``: DESIGN.md section 17); ``--weight_decay``, ``--clip_grad``, ``--ema`` and ``--lr_schedule`` add the usual
fine-tuning recipe to the fused optimizer step (without them the run is the reference's Adam(lr)); ``--diff_maps`` writes its difference-map and overlay dumps (:404-449); its plots (:468-611) are visualisation and out of scope.
"""
import argparse
import contextlib
import gc
import os
import time

import torch
from torch.utils.data import DataLoader, Subset

from unet_dc_segmentation_amd import dp as dpmod
from utils.data_loader import SegmentationDataset, SyntheticDropletDataset, TrainAugment
from utils.metrics_DC import combined_loss, dice_coef, focal_dice_loss, metrics_from_counts


def build_parser(arch="unetdc", epochs=15, ckpt="best_UNetDC_focal_model.pth", loss="focal_dice"):
    p = argparse.ArgumentParser("Train the U-Net(-DC) segmentation model")
    p.add_argument("--image_dir")
    p.add_argument("--mask_dir")
    p.add_argument("--mask_polygons", metavar="PATH",
                   help="with --device_data, instead of --mask_dir: polygon annotations -- a directory with NAME.geojson per "
                        "image, or a COCO .json file matched by the stem of file_name.  The mask of an image is its filled "
                        "polygons (labels > 0; the exact rule of DESIGN.md section 28, filled on the HIP device at the image's "
                        "own size), and is cached like a mask file from there")
    p.add_argument("--synthetic", action="store_true", help="seeded synthetic droplet tiles instead of a dataset")
    p.add_argument("--synthetic_len", type=int, default=64)
    p.add_argument("--arch", default=arch, choices=["unetdc", "unet"])
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--img_size", type=int, default=512)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--epochs", type=int, default=epochs)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--patience", type=int, default=5)
    p.add_argument("--loss", default=loss, choices=["focal_dice", "bce_dice"])
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    p.add_argument("--steps", type=int, default=0, help="max training steps per epoch (0 = all)")
    p.add_argument("--optimizer", default="hip", choices=["hip", "torch"],
                   help="Adam implementation on a GPU: hip = fused step + weight re-pack kernel, torch = torch.optim.Adam")
    p.add_argument("--weight_decay", type=float, default=0.0, metavar="WD",
                   help="decoupled weight decay (torch.optim.AdamW's rule) in the fused step, on the conv, transposed-conv and "
                        "head weights; biases and the BatchNorm affine are left alone (DESIGN.md section 22); default 0")
    p.add_argument("--decay_all", action="store_true", help="with --weight_decay: decay every parameter (torch's one-group AdamW)")
    p.add_argument("--clip_grad", type=float, default=None, metavar="N",
                   help="clip the global L2 norm of the gradient to N (torch.nn.utils.clip_grad_norm_'s rule; the norm stays on "
                        "the device) and drop a step whose gradient holds an inf or a NaN; the epoch records gain "
                        "grad_norm_mean, clipped_steps and skipped_steps")
    p.add_argument("--ema", type=float, default=None, metavar="D",
                   help="keep an exponential moving average of the weights with decay D (warm-up min(D, (1 + t) / (10 + t))); "
                        "validation, early stopping, the saved checkpoint, the final test and --calibrate_thresh use the "
                        "averaged weights")
    p.add_argument("--lr_schedule", default="constant", choices=["constant", "cosine", "plateau"],
                   help="cosine: per optimizer step over the planned steps of the run, down to --lr_min; plateau: "
                        "ReduceLROnPlateau(mode='min', factor=0.5, patience=5) on the epoch's validation loss (the scheduler the "
                        "reference declares); the epoch records gain lr")
    p.add_argument("--warmup_steps", type=int, default=0, metavar="N", help="linear learning-rate warm-up over the first N steps")
    p.add_argument("--lr_min", type=float, default=0.0, help="with --lr_schedule cosine / plateau: the floor of the rate")
    p.add_argument("--workers", type=int, default=4)
    from utils.intensity_window import add_flags
    add_flags(p)
    p.add_argument("--device_data", action="store_true",
                   help="decode and preprocess every image once into a cache on the HIP device and augment each batch there "
                        "(csrc/augment.hip; its own counter-based random stream); --workers is ignored")
    p.add_argument("--crop", type=int, nargs="?", const=512, default=None, metavar="S",
                   help="with --device_data: train at native resolution on random S x S windows of images cached at their own "
                        "size, cut and augmented on the HIP device (csrc/crop.hip, DESIGN.md section 16); validation and test "
                        "run on the windows of utils.crops.eval_plan.  S: a multiple of 16 in 32..1024, 512 without S; "
                        "--img_size is not used")
    p.add_argument("--crops_per_image", type=int, default=1, metavar="R",
                   help="with --crop: R random windows of every training image per epoch (default 1)")
    p.add_argument("--crop_scale", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="with --crop: scale jitter.  Every training window is cut with a source side T drawn uniformly from the "
                        "integers ceil(LO * S) .. floor(HI * S) and resampled to S x S in the crop kernel (8-bit bilinear, masks "
                        "nearest); 0.5 <= LO <= 1 <= HI <= 2, default off.  Validation, test and --calibrate_thresh stay at "
                        "scale 1")
    p.add_argument("--crop_fg", type=float, default=0.0, metavar="P",
                   help="with --crop: with probability P a training window is placed so that it contains a uniformly chosen "
                        "foreground pixel of its image, otherwise uniformly as without the flag; 0 <= P <= 1, default 0")
    p.add_argument("--border_weight", type=float, nargs="?", const=10.0, default=None, metavar="W0",
                   help="with --loss focal_dice: weight the pixel-wise focal term of the TRAINING loss by the U-Net separation map "
                        "1 + W0 * exp(-(d1 + d2)^2 / (2 S^2)) on the background between two droplets (d1, d2: distances to the "
                        "nearest and second-nearest droplet), built per batch from the masks (csrc/border.hip on the HIP device, "
                        "DESIGN.md section 19); W0 >= 0, 10 without W0, default off.  Dice, the validation and test losses, the "
                        "metrics, early stopping and --calibrate_thresh stay unweighted")
    p.add_argument("--border_sigma", type=float, default=None, metavar="S",
                   help="with --border_weight: the width S of the separation term in pixels (default 5)")
    p.add_argument("--border_radius", type=int, default=None, metavar="R",
                   help="with --border_weight: droplets further than R pixels away do not count (1..64, default ceil(4 S))")
    p.add_argument("--boundary", type=int, nargs="?", const=64, default=None, metavar="R",
                   help="the final test evaluation also reports boundary accuracy: pooled HD95, average symmetric surface "
                        "distance, surface Dice (nsd) and boundary F at 1, 2, 3 pixels of the thresholded predictions against "
                        "the masks (both binary; distances beyond R pixels, 1..64, 64 without R, count as far)")
    p.add_argument("--diff_maps", nargs="?", const=".", default=None, metavar="DIR",
                   help="the final test evaluation also writes, per test image at the network's resolution, "
                        "DIR/differences_map_test/NAME_diffmap.png (yellow: predicted and annotated, red: only annotated, green: "
                        "only predicted) and DIR/overlay_diff_test/NAME_overlay.png (that map over the network's input), and "
                        "reports the 8-connected yellow / red / green / black regions summed over the test set (region-level "
                        "TP / FN / FP / TN; DESIGN.md section 25); DIR is the working directory without DIR")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--ckpt_path", default=ckpt)
    p.add_argument("--no_test_eval", dest="test_eval", action="store_false",
                   help="skip the evaluation of the best checkpoint on the held-out test split after training")
    p.add_argument("--calibrate_thresh", type=int, nargs="?", const=100, metavar="K",
                   help="after the final test evaluation, run the validation split once more with the weights that evaluation "
                        "used and report the Dice-optimal probability threshold among k / K, k = 0..K-1 (K in 1..1024, 100 "
                        "without K; csrc/sweep.hip on the HIP device).  This is Dice POOLED OVER ALL PIXELS of the split, not "
                        "the per-batch mean Dice the epochs print")
    p.add_argument("--tta", type=int, nargs="?", const=8, default=1, metavar="N",
                   help="test-time augmentation in the final test evaluation and in --calibrate_thresh only: the network's mean "
                        "over N flipped and rotated variants of every input (N in 1, 2, 4, 8; 8 without N; DESIGN.md section "
                        "17), --batch items per forward.  The training and validation loops do not change")
    p.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    return p


def intensity_spec(args):
    """--intensity_window / --intensity_levels / --page -> utils.intensity_window.WindowSpec, or None without a window flag (DESIGN.md
    section 29): deep images are then windowed to 8 bits in front of the rolling ball, on the device with --device_data."""
    from utils import intensity_window as iw
    try:
        return iw.spec_from_flags(args.intensity_window, args.intensity_levels, args.page)
    except ValueError as e:
        raise SystemExit(str(e))


def make_datasets(args):
    if args.synthetic:
        full = SyntheticDropletDataset(args.synthetic_len, args.img_size, args.in_channels, seed=args.seed)
        n = len(full)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(args.seed)).tolist()
        n_test, n_val = max(1, n // 5), max(1, n // 5)                    # 60/20/20 like the reference
        return (Subset(full, idx[n_test + n_val:]), Subset(full, idx[n_test:n_test + n_val]),
                Subset(full, idx[:n_test]))
    tr, va, te = split_files(args)
    mk = lambda pair, tf: SegmentationDataset(args.image_dir, args.mask_dir, pair[0], pair[1], transform=tf,  # noqa: E731
                                              size=args.img_size, intensity=intensity_spec(args))
    return mk(tr, TrainAugment(args.seed)), mk(va, None), mk(te, None)


def split_files(args):
    """(image names, mask names) of the train, validation and test splits of --image_dir / --mask_dir."""
    if not args.image_dir or not (args.mask_dir or args.mask_polygons):
        raise SystemExit("--image_dir and --mask_dir are required unless --synthetic is given")
    exts = (".png", ".jpg", ".jpeg", ".tif")
    imgs = sorted(f for f in os.listdir(args.image_dir) if f.lower().endswith(exts))
    # --mask_polygons: the annotation of an image is found by the image's own name
    masks = list(imgs) if args.mask_polygons else sorted(f for f in os.listdir(args.mask_dir) if f.lower().endswith(exts))
    assert len(imgs) == len(masks), "Mismatch between the number of images and masks!"
    idx = torch.randperm(len(imgs), generator=torch.Generator().manual_seed(args.seed)).tolist()
    n_test = max(1, len(imgs) // 5)
    n_val = max(1, (len(imgs) - n_test) // 4)
    pick = lambda ids: ([imgs[i] for i in ids], [masks[i] for i in ids])   # noqa: E731
    return pick(idx[n_test + n_val:]), pick(idx[n_test:n_test + n_val]), pick(idx[:n_test])


def make_device_loaders(args, rank, world, device):
    """--device_data: (train, validation, test) loaders over caches on the device (unet_dc_segmentation_amd/device_data.py).
    A data-parallel rank caches only its training shard, the one the host path's Subset picks."""
    from unet_dc_segmentation_amd.device_data import DeviceEvalLoader, DeviceImageCache, DeviceTrainLoader
    if args.synthetic:
        raise SystemExit("--device_data caches the files of --image_dir / --mask_dir; --synthetic tiles need no cache")
    tr, va, te = split_files(args)
    polygons = None
    if args.mask_polygons:                               # every annotation read, checked and packed before any cache is built
        from utils import polygon_masks as pm
        try:
            found = pm.find_polygons(args.mask_polygons, [os.path.join(args.image_dir, n) for n in tr[0] + va[0] + te[0]])
            polygons = {os.path.basename(k): load()[0] for k, load in found.items()}
        except pm.PolygonError as e:
            raise SystemExit(f"--mask_polygons: {e}")
    ids = list(range(len(tr[0])))
    if world > 1:
        per_rank = len(ids) // world
        ids = list(range(rank, per_rank * world, world))
    if args.crop is not None:
        from unet_dc_segmentation_amd.device_data import DeviceCropEvalLoader, DeviceCropTrainLoader, DeviceNativeCache
        native = lambda names, masks, fg=False: DeviceNativeCache(args.image_dir, args.mask_dir, names,  # noqa: E731
                                                                  device=device, mask_names=masks, keep_foreground=fg,
                                                                  mask_polygons=polygons, intensity=intensity_spec(args))
        train = DeviceCropTrainLoader(native([tr[0][i] for i in ids], [tr[1][i] for i in ids], args.crop_fg > 0), args.batch,
                                      args.crop, args.seed, ids, args.crops_per_image, scale=args.crop_scale, p_fg=args.crop_fg)
        return (train, DeviceCropEvalLoader(native(*va), args.batch, args.crop),
                DeviceCropEvalLoader(native(*te), args.batch, args.crop))
    cache = lambda names, masks: DeviceImageCache(args.image_dir, args.mask_dir, names, args.img_size,  # noqa: E731
                                                  device=device, mask_names=masks, mask_polygons=polygons,
                                                  intensity=intensity_spec(args))
    train = DeviceTrainLoader(cache([tr[0][i] for i in ids], [tr[1][i] for i in ids]), args.batch, args.seed, ids)
    return train, DeviceEvalLoader(cache(*va), args.batch), DeviceEvalLoader(cache(*te), args.batch)


def check_crop_flags(args):
    """--crop / --crops_per_image / --crop_scale / --crop_fg: every refusal is raised here, before any file is read."""
    from utils.crops import MAX_CROP, MAX_SCALE, MIN_CROP, MIN_SCALE
    if args.crop_scale is not None:
        lo, hi = args.crop_scale
        if not (MIN_SCALE <= lo <= 1.0 <= hi <= MAX_SCALE):              # (also refuses LO > HI and a NaN)
            raise SystemExit(f"--crop_scale LO HI: {MIN_SCALE} <= LO <= 1 <= HI <= {MAX_SCALE}, not {lo} {hi}")
    if not 0.0 <= args.crop_fg <= 1.0:
        raise SystemExit(f"--crop_fg P: P must be in 0..1, not {args.crop_fg}")
    if args.crop is None:
        if args.crops_per_image != 1:
            raise SystemExit("--crops_per_image needs --crop")
        if args.crop_scale is not None:
            raise SystemExit("--crop_scale needs --crop")
        if args.crop_fg != 0.0:
            raise SystemExit("--crop_fg needs --crop")
        return
    if args.crop % 16 or not MIN_CROP <= args.crop <= MAX_CROP:
        raise SystemExit(f"--crop S: S must be a multiple of 16 in {MIN_CROP}..{MAX_CROP}, not {args.crop}")
    if args.crops_per_image < 1:
        raise SystemExit(f"--crops_per_image R: R must be at least 1, not {args.crops_per_image}")
    if args.synthetic:
        raise SystemExit("--crop cuts windows out of the files of --image_dir / --mask_dir and cannot run with --synthetic")
    if not args.device_data:
        raise SystemExit("--crop needs --device_data: the windows are cut from a cache on the HIP device")
    if torch.device(args.device).type != "cuda":
        raise SystemExit(f"--crop cuts and augments its windows on the HIP device and cannot run on --device {args.device}")
    if args.in_channels != 3:
        raise SystemExit(f"--crop caches RGB images and cannot run with --in_channels {args.in_channels}")


def check_border_flags(parser, args):
    """--border_weight / --border_sigma / --border_radius: parser errors, raised before anything else runs.
    -> None without --border_weight, else (w0, sigma, radius)."""
    from utils.border_weights import DEFAULT_SIGMA, check_params
    if args.border_weight is None:
        if args.border_sigma is not None or args.border_radius is not None:
            parser.error("--border_sigma and --border_radius need --border_weight")
        return None
    if args.loss != "focal_dice":
        parser.error(f"--border_weight weights the focal term and cannot run with --loss {args.loss}")
    try:
        return check_params(args.border_weight, DEFAULT_SIGMA if args.border_sigma is None else args.border_sigma,
                            args.border_radius)
    except ValueError as e:
        parser.error(f"--border_weight W0 / --border_sigma S / --border_radius R: {e}")


def check_optim_flags(args):
    """--weight_decay / --decay_all / --clip_grad / --ema / --lr_schedule / --warmup_steps / --lr_min: every refusal is raised
    here, before any file is read.  -> True when one of the three optimizer flags is given (the recipe of FusedAdam)."""
    recipe = [f for f, on in (("--weight_decay", args.weight_decay != 0.0), ("--clip_grad", args.clip_grad is not None),
                              ("--ema", args.ema is not None)) if on]
    if not args.weight_decay >= 0.0:
        raise SystemExit(f"--weight_decay WD: WD must be >= 0, not {args.weight_decay}")
    if args.decay_all and not args.weight_decay:
        raise SystemExit("--decay_all needs --weight_decay")
    if args.clip_grad is not None and not args.clip_grad > 0.0:
        raise SystemExit(f"--clip_grad N: N must be > 0, not {args.clip_grad}")
    if args.ema is not None and not 0.0 <= args.ema < 1.0:
        raise SystemExit(f"--ema D: D must be in [0, 1), not {args.ema}")
    if args.warmup_steps < 0:
        raise SystemExit(f"--warmup_steps N: N must be >= 0, not {args.warmup_steps}")
    if not 0.0 <= args.lr_min <= args.lr:
        raise SystemExit(f"--lr_min: must be in 0..--lr, not {args.lr_min}")
    if args.lr_min and args.lr_schedule == "constant":
        raise SystemExit("--lr_min needs --lr_schedule cosine or plateau")
    if recipe and args.optimizer == "torch":
        raise SystemExit(f"{', '.join(recipe)}: weight decay, clipping and the EMA live in the fused optimizer step "
                         "(unet_dc_segmentation_amd/optim.py) and cannot run with --optimizer torch; drop that flag "
                         "(--optimizer hip is the default; on --device cpu it runs the same rules in PyTorch)")
    return bool(recipe)


class History(list):
    """Per-epoch records of main(); ``.test`` holds the held-out-split results of the final evaluation (None if skipped),
    ``.calibration`` the result of --calibrate_thresh (None without the flag), ``.tta`` the number of variants both were
    computed with (--tta; 1 = the plain forward)."""
    test = None
    calibration = None
    tta = 1


def predict_eval(model, images, tta, batch):
    """The probabilities the final evaluations read: the plain forward, or with --tta N the mean over the N variants of every
    image (unet_dc_segmentation_amd/tta.py on the HIP device, utils/tta.py on the CPU), `batch` items per forward."""
    if tta == 1:
        return model(images)
    if images.is_cuda:
        from unet_dc_segmentation_amd.tta import predict_tta
        return predict_tta(model, images, tta, batch)
    from utils.tta import predict_tta_cpu
    return predict_tta_cpu(model, images, tta, batch)


def pool_boundary(yp, yt, radius, state=None):
    """--boundary: adds the surface distances between the binary predictions yp and masks yt (bool
    [N, 1, H, W], a label map with K = 1 on either side) into state = (hist, dmax), which it returns (a new one from None).  On
    the HIP device the pair are device tensors and every image adds into them (unetdc_boundary_distances, nothing waits); on the
    CPU they are numpy arrays and utils.droplet_boundary does the same sums."""
    n = len(yp)
    if yp.is_cuda:
        from unet_dc_segmentation_amd.evaluate import boundary_batch
        if state is None:
            state = (torch.zeros(2, radius * radius + 2, dtype=torch.int64, device=yp.device),
                     torch.full((2,), -1, dtype=torch.int32, device=yp.device))
        a, b = yp[:, 0].to(torch.int32).contiguous(), yt[:, 0].to(torch.int32).contiguous()
        boundary_batch(list(a), [1] * n, list(b), [1] * n, radius, hist=state[0], dmax=state[1], objects=False)
        return state
    import numpy as np
    from utils.droplet_boundary import boundary_record_numpy
    if state is None:
        state = (np.zeros((2, radius * radius + 2), np.int64), np.full(2, -1, np.int64))
    for a, b in zip(yp[:, 0].numpy(), yt[:, 0].numpy()):
        rec = boundary_record_numpy(a.astype(np.int32), 1, b.astype(np.int32), 1, radius, objects=False)
        state = (state[0] + rec["hist"], np.maximum(state[1], rec["dmax"]))
    return state


def boundary_report(state, radius):
    """The pooled planes of pool_boundary -> {"R", "hist", "dmax", and the columns of utils.droplet_boundary.boundary_columns}."""
    from utils.droplet_boundary import DEFAULT_TOLS, boundary_columns
    hist, dmax = state
    if torch.is_tensor(hist):
        from unet_dc_segmentation_amd.evaluate import boundary_result
        hist, dmax = boundary_result(hist, dmax)
    tols = tuple(t for t in DEFAULT_TOLS if t <= radius)
    return {"R": radius, "hist": hist, "dmax": dmax, **boundary_columns(hist, dmax, radius, tols)}


def dump_diff_maps(images, yp, yt, names, out_dir):
    """--diff_maps for one test batch: per image the difference map of the thresholded prediction against the mask (DESIGN.md
    section 25) as out_dir/differences_map_test/NAME_diffmap.png and, painted on (image * 255) truncated to uint8 (reference
    :439-440), out_dir/overlay_diff_test/NAME_overlay.png, both at the network's resolution.  On the HIP device the regions and
    both pictures come from unetdc_diff_regions / unetdc_diff_paint (one wait per batch), on the CPU from
    utils/difference_map.py.  -> the utils.difference_map.image_columns of every image."""
    from PIL import Image
    from utils import difference_map as dmap
    preds, gts = yp[:, 0].to(torch.uint8).contiguous(), yt[:, 0].to(torch.uint8).contiguous()
    rgbs = (images * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    if images.is_cuda:
        from unet_dc_segmentation_amd.evaluate import diff_regions_batch
        recs = diff_regions_batch(list(preds), list(gts), 1, list(rgbs), paint=True)
        for r in recs:
            r["diff"], r["overlay"] = r["diff"].cpu().numpy(), r["overlay"].cpu().numpy()
    else:
        recs = []
        for p, g, rgb in zip(preds.numpy(), gts.numpy(), rgbs.numpy()):
            recs.append({**dmap.diff_regions_numpy(p, g, 1), "diff": dmap.difference_map_rgb(p, g),
                         "overlay": dmap.overlay_difference(rgb, p, g)})
    for name, r in zip(names, recs):
        Image.fromarray(r["diff"]).save(os.path.join(out_dir, "differences_map_test", f"{name}_diffmap.png"))
        Image.fromarray(r["overlay"]).save(os.path.join(out_dir, "overlay_diff_test", f"{name}_overlay.png"))
    return [dmap.image_columns(r) for r in recs]


def evaluate_test(model, loader, criterion, device, tta=1, items=8, boundary=None, diff_maps=None):
    """The reference's final test pass (train_DC_focal.py:365-402, :452-467): mean loss and Dice over the batches, pixel accuracy
    over all pixels, and calculate_metrics() on the thresholded predictions.  Sums stay on the device (one read-back), like the
    training loop's.  tta, items: the number of variants of --tta and of items per forward.
    boundary (a radius): also "boundary", the pooled boundary_report of the thresholded predictions against the masks.
    diff_maps (a directory): the reference's difference-map and overlay dumps (:404-449) under it, at the network's resolution,
    named after the loader's file names (test_%05d where it yields none), and "diff_regions", the image_columns of
    utils/difference_map.py summed over the test set (its *_blobs are the reference's count_color_regions_in_memory)."""
    model.eval()
    loss_t = torch.zeros((), dtype=torch.float64, device=device)
    dice_t = torch.zeros((), dtype=torch.float64, device=device)
    cm_t = torch.zeros(4, dtype=torch.int64, device=device)           # tn, fp, fn, tp
    bstate, diff_rows, seen = None, [], 0
    if diff_maps is not None:
        for sub in ("differences_map_test", "overlay_diff_test"):
            os.makedirs(os.path.join(diff_maps, sub), exist_ok=True)
    with torch.no_grad():
        for batch in loader:
            images, masks = batch[0].float().to(device), batch[1].float().to(device)
            outputs = predict_eval(model, images, tta, items)
            loss_t += criterion(outputs, masks).double()
            pred = (outputs > 0.3).float()
            dice_t += dice_coef(masks, pred).double()
            yt, yp = masks > 0.5, pred > 0.5
            cm_t += torch.stack([(~yp & ~yt).sum(), (yp & ~yt).sum(), (~yp & yt).sum(), (yp & yt).sum()])
            if boundary is not None:
                bstate = pool_boundary(yp, yt, boundary, bstate)
            if diff_maps is not None:
                names = batch[-1] if len(batch) > 2 and isinstance(batch[-1], (list, tuple)) and \
                    all(isinstance(q, str) for q in batch[-1]) else None
                names = [os.path.splitext(q)[0] for q in names] if names else [f"test_{seen + j:05d}" for j in range(len(images))]
                diff_rows += dump_diff_maps(images, yp, yt, names, diff_maps)
                seen += len(images)
    nb = max(1, len(loader))
    tn, fp, fn, tp = (int(v) for v in cm_t.tolist())
    precision, recall, f1, specificity, cm = metrics_from_counts(tn, fp, fn, tp)     # = calculate_metrics() on the label arrays
    total = max(1, tn + fp + fn + tp)
    out = dict(test_loss=float(loss_t.item()) / nb, test_dice=float(dice_t.item()) / nb, test_acc=(tn + tp) / total,
               precision=precision, recall=recall, f1=f1, specificity=specificity, confusion=cm.tolist())
    if bstate is not None:
        out["boundary"] = boundary_report(bstate, boundary)
    if diff_maps is not None:
        from utils.difference_map import sum_image_columns
        out["diff_regions"] = sum_image_columns(diff_rows)
    return out


def calibrate_threshold(model, loader, K, device, tta=1, items=8):
    """--calibrate_thresh: the pixel confusion matrix of `probabilities > k / K` against the masks (> 0.5) of every batch of
    `loader`, for all k at once (identity geometry, nearest rule).  On the HIP device every batch adds
    into one device histogram (unetdc_thresh_sweep) and the host copies it once; on the CPU utils.threshold_sweep does the
    same sums.  tta, items: the number of variants of --tta and of items per forward (a threshold calibrated without --tta is
    not the one to apply with it).
    -> {K, best_dice_threshold, best_dice, average_precision, hist}."""
    from utils.threshold_sweep import sweep_hist_numpy, sweep_table
    model.eval()
    hist = None
    with torch.no_grad():
        for batch in loader:
            images, masks = batch[0].float().to(device), batch[1].float().to(device)
            probs = predict_eval(model, images, tta, items)[:, 0].float()
            gts = (masks[:, 0] > 0.5).to(torch.uint8)
            hw = tuple(gts.shape[1:])
            if probs.is_cuda:
                from unet_dc_segmentation_amd.evaluate import sweep_batch
                hist = sweep_batch(probs, gts, [hw] * len(probs), K, hist=hist, linear=False)
            else:
                for p2, g in zip(probs.numpy(), gts.numpy()):
                    h = sweep_hist_numpy(p2, g, hw, K, linear=False)
                    hist = h if hist is None else hist + h
    if torch.is_tensor(hist):
        from unet_dc_segmentation_amd.evaluate import sweep_result
        hist = sweep_result(hist)
    t = sweep_table(hist)
    k = t["best_dice_k"]
    return dict(K=K, best_dice_threshold=float(t["threshold"][k]), best_dice=float(t["dice"][k]),
                average_precision=t["average_precision"], hist=hist)


def main(argv=None, parser=None):
    parser = parser or build_parser()
    args = parser.parse_args(argv)
    border = check_border_flags(parser, args)
    if args.calibrate_thresh is not None and not 1 <= args.calibrate_thresh <= 1024:
        raise SystemExit("--calibrate_thresh K: K must be in 1..1024")
    check_crop_flags(args)
    intensity_spec(args)                                 # checked before anything is read
    if args.mask_polygons and args.mask_dir:
        raise SystemExit("--mask_polygons and --mask_dir are two sources of the same masks: give one")
    if args.mask_polygons and not args.device_data:
        raise SystemExit("--mask_polygons needs --device_data: the polygons are filled on the HIP device into its cache "
                         "(the host loader reads mask files only)")
    recipe = check_optim_flags(args)
    if args.boundary is not None and not 1 <= args.boundary <= 64:
        raise SystemExit("--boundary R: R must be in 1..64")
    if args.diff_maps is not None and args.in_channels != 3:
        raise SystemExit(f"--diff_maps paints on RGB inputs and cannot run with --in_channels {args.in_channels}")
    from utils.tta import TTA_SIZES
    if args.tta not in TTA_SIZES:
        raise SystemExit(f"--tta N: N must be one of {', '.join(map(str, TTA_SIZES))}, not {args.tta}")
    rank, local, world = dpmod.init_from_env()
    device = torch.device(args.device if args.device != "cuda" else f"cuda:{local}")
    if args.device_data and device.type != "cuda":
        raise SystemExit(f"--device_data keeps the data set on the HIP device and cannot run on --device {args.device}")
    if device.type == "cuda":
        torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    if args.arch == "unetdc":
        from models.model_2 import UNetDC as Net
    else:
        from models.model import UNet as Net
    model = Net(in_channels=args.in_channels, out_channels=1).to(device)
    model.set_compute_dtype(args.dtype)
    wrapper = dpmod.DataParallel(model) if world > 1 else None
    if args.loss == "focal_dice":
        criterion = lambda pred, tgt: focal_dice_loss(pred, tgt, alpha=1.0, gamma=2.0, ratio=0.3)  # noqa: E731
    else:
        criterion = combined_loss
    # the training loss alone takes the separation weights; validation, test and early stopping keep `criterion`
    train_criterion = criterion
    if border is not None:
        from unet_dc_segmentation_amd.border import border_weights

        def train_criterion(pred, tgt):
            return focal_dice_loss(pred, tgt, alpha=1.0, gamma=2.0, ratio=0.3, weight=border_weights(tgt, *border))
    # same update as the reference's torch.optim.Adam(lr) (train_DC_focal.py:224).  On the HIP path: one kernel that also
    # rewrites the packed weight images (unet_dc_segmentation_amd/optim.py); --optimizer torch keeps torch.optim.Adam
    if recipe:
        # --weight_decay / --clip_grad / --ema: the recipe of the fused step; on CPU tensors the same
        # class runs the same rules in PyTorch
        from unet_dc_segmentation_amd.optim import FusedAdam
        optimizer = FusedAdam(model, lr=args.lr, weight_decay=args.weight_decay, decay="all" if args.decay_all else "weights",
                              clip_norm=args.clip_grad, ema_decay=args.ema)
    elif device.type == "cuda" and args.optimizer == "hip":
        from unet_dc_segmentation_amd.optim import FusedAdam
        optimizer = FusedAdam(model, lr=args.lr)
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=args.lr, fused=next(model.parameters()).is_cuda)

    if args.device_data:
        train_loader, val_loader, test_loader = make_device_loaders(args, rank, world, device)
        train_ds, val_ds, test_ds = train_loader.dataset, val_loader.dataset, test_loader.dataset
    else:
        train_ds, val_ds, test_ds = make_datasets(args)
        if world > 1:
            # each rank draws its own shard; shards are truncated to EQUAL length (as DistributedSampler with
            # drop_last does) so that every rank runs the same number of steps -- an extra step on one rank would
            # leave its gradient all-reduce without partners
            per_rank = len(train_ds) // world
            train_ds = Subset(train_ds, list(range(rank, per_rank * world, world)))
        pin = device.type == "cuda"
        # worker processes live across epochs (re-spawning them costs seconds per epoch: an interpreter + torch import each)
        keep = args.workers > 0
        # no drop_last, like the reference's loader (train_DC_focal.py:200): the ragged last batch trains too (the engines of both
        # batch shapes stay alive, unet.py::_engine_for; under data parallelism the shards are equal, so is every rank's last batch)
        train_loader = DataLoader(train_ds, batch_size=args.batch, shuffle=True, num_workers=args.workers,
                                  pin_memory=pin, persistent_workers=keep)
        val_loader = DataLoader(val_ds, batch_size=args.batch, shuffle=False, num_workers=args.workers, pin_memory=pin,
                                persistent_workers=keep)
    if rank == 0 and args.crop is not None:
        print(f"--crop {args.crop}: {train_loader.samples} random {args.crop} x {args.crop} windows/rank and epoch at native "
              f"resolution, {len(val_loader.windows)} validation windows; --img_size {args.img_size} is not used")
        if train_loader.scaled:
            from utils.crops import t_range
            tlo, thi = t_range(args.crop, args.crop_scale) if args.crop_scale is not None else (args.crop, args.crop)
            print(f"--crop_scale / --crop_fg: source windows of side T in {tlo}..{thi} resampled to {args.crop} x {args.crop} "
                  f"on the device, a window placed on a foreground pixel with probability P = {args.crop_fg:g}; validation "
                  f"and test at scale 1")
    if rank == 0 and border is not None:
        print(f"--border_weight {border[0]:g}: training loss with the focal term weighted by 1 + {border[0]:g} * "
              f"exp(-(d1 + d2)^2 / (2 * {border[1]:g}^2)) between droplets at most {border[2]} px apart, built per batch on "
              f"{'the HIP device' if device.type == 'cuda' else 'the host'}; validation and test losses stay unweighted")
    if rank == 0:
        print(f"Training set: {len(train_ds)} images/rank, validation set: {len(val_ds)} images, "
              f"{world} rank(s), device {device}, compute {args.dtype}")

    # learning-rate schedule: a host number set on the group before every step (the step kernel takes lr by value); None = the
    # constant rate of the reference, nothing is touched
    schedule, opt_step = None, 0
    if args.lr_schedule != "constant" or args.warmup_steps:
        from utils.lr_schedule import LRSchedule
        per_epoch = min(len(train_loader), args.steps or len(train_loader))
        try:
            schedule = LRSchedule(args.lr_schedule, args.lr, args.epochs * per_epoch, args.warmup_steps, args.lr_min)
        except ValueError as e:
            raise SystemExit(f"--lr_schedule {args.lr_schedule}: {e}")
    # --ema: validation, the checkpoint and the final evaluations read the averaged weights
    ema_weights = optimizer.ema_weights if args.ema is not None else contextlib.nullcontext
    stats_prev = dict(steps=0, clipped=0, skipped=0, norm_sum=0.0)

    best_dice, patience_counter = 0.0, 0
    saved_this_run = False          # the final test evaluation only reloads a checkpoint THIS run wrote
    history = History()
    history.tta = args.tta
    for epoch in range(args.epochs):
        model.train()
        # the per-step metrics of train_DC_focal.py:256-262 are ACCUMULATED ON THE DEVICE (fp64 / int64: the same values added in
        # the same order as the reference's Python floats) and read back once per epoch: three .item() calls per step would
        # stall the launch queue three times per step
        tr_loss_t = torch.zeros((), dtype=torch.float64, device=device)
        tr_dice_t = torch.zeros((), dtype=torch.float64, device=device)
        correct_t = torch.zeros((), dtype=torch.int64, device=device)
        total = 0
        t0, seen = time.time(), 0
        for step, batch in enumerate(train_loader):
            if args.steps and step >= args.steps:
                break
            images, masks = batch[0].float().to(device, non_blocking=True), batch[1].float().to(device, non_blocking=True)
            optimizer.zero_grad()
            outputs = model(images)
            loss = train_criterion(outputs, masks)
            loss.backward()
            if wrapper is not None and not images.is_cuda:
                wrapper.sync_gradients()                    # ATen-CPU path: explicit all-reduce
            if schedule is not None:
                optimizer.param_groups[0]["lr"] = schedule.lr_at(opt_step)
                opt_step += 1
            optimizer.step()
            with torch.no_grad():
                tr_loss_t += loss.detach().double()
                pred = (outputs > 0.3).float()
                tr_dice_t += dice_coef(masks, pred).double()
                correct_t += (pred == masks).sum()
            total += masks.numel()
            seen += images.shape[0]
            if epoch == 0 and step == 0:
                # Everything alive after the first step (torch, the model, the engine's buffers and descriptor tables, the
                # loader's workers) stays alive for the whole run: move it out of the cyclic collector's generations, so that
                # the full collections Python triggers during training scan the few objects of the loop instead of torch's
                # whole heap (a generation-2 pass there was measured at 40-60 ms: five training steps of host time).
                gc.collect()
                gc.freeze()
        nb = max(1, min(len(train_loader), args.steps or len(train_loader)))
        tr_loss, tr_dice, correct = float(tr_loss_t.item()), float(tr_dice_t.item()), int(correct_t.item())   # (waits for the epoch's work)
        dt = time.time() - t0
        clip_rec = {}
        if args.clip_grad is not None:
            # one read of the optimizer's device record per epoch, next to the read-back above (the queue is drained anyway)
            s = optimizer.recipe_stats()
            s["norm_sum"] = (s["grad_norm_mean"] or 0.0) * (s["steps"] - s["skipped"])
            done = (s["steps"] - s["skipped"]) - (stats_prev["steps"] - stats_prev["skipped"])
            clip_rec = dict(grad_norm_mean=(s["norm_sum"] - stats_prev["norm_sum"]) / done if done else 0.0,
                            clipped_steps=s["clipped"] - stats_prev["clipped"], skipped_steps=s["skipped"] - stats_prev["skipped"])
            stats_prev = s
        # -------- validation --------
        if wrapper is not None:
            wrapper.broadcast_buffers()                     # rank 0's BatchNorm running statistics everywhere
        model.eval()
        va_loss_t = torch.zeros((), dtype=torch.float64, device=device)
        va_dice_t = torch.zeros((), dtype=torch.float64, device=device)
        vc_t = torch.zeros((), dtype=torch.int64, device=device)
        vt = 0
        with torch.no_grad(), ema_weights():
            for batch in val_loader:
                images, masks = batch[0].float().to(device), batch[1].float().to(device)
                outputs = model(images)
                va_loss_t += criterion(outputs, masks).double()
                pred = (outputs > 0.3).float()
                va_dice_t += dice_coef(masks, pred).double()
                vc_t += (pred == masks).sum()
                vt += masks.numel()
        va_loss, va_dice, vc = float(va_loss_t.item()), float(va_dice_t.item()), int(vc_t.item())
        nv = max(1, len(val_loader))
        rec = dict(epoch=epoch + 1, train_loss=tr_loss / nb, val_loss=va_loss / nv, train_dice=tr_dice / nb,
                   val_dice=va_dice / nv, train_acc=correct / max(total, 1), val_acc=vc / max(vt, 1),
                   images_per_sec=seen * world / max(dt, 1e-9))
        if args.crop is not None and train_loader.scaled:
            rec["fg_windows"] = int(train_loader.fg_windows)              # (this rank's windows)
        if schedule is not None:
            rec["lr"] = float(optimizer.param_groups[0]["lr"])            # the rate of the epoch's last step
            # plateau: every rank steps on rank 0's validation loss, so all ranks keep the same rate
            schedule.epoch_end(dpmod.broadcast_scalar(rec["val_loss"], device) if world > 1 else rec["val_loss"])
        rec.update(clip_rec)
        if world > 1:
            # replicas must stay identical: one checksum per rank and epoch (compared by tests/test_dp_gloo.py)
            with torch.no_grad():
                rec["param_checksum"] = float(sum(p.double().sum() for p in model.parameters()))
            # early stopping / checkpointing are decided from rank 0's validation Dice on every rank, so all ranks
            # leave the loop in the same epoch (a rank that stopped alone would strand the others in all_reduce)
            rec["val_dice"] = dpmod.broadcast_scalar(rec["val_dice"], device)
        history.append(rec)
        if rank == 0:
            print(f"Epoch {epoch + 1}/{args.epochs} | Train Loss: {rec['train_loss']:.4f}, Val Loss: {rec['val_loss']:.4f}, "
                  f"Train Dice: {rec['train_dice']:.4f}, Val Dice: {rec['val_dice']:.4f}")
            print(f"Train Acc: {rec['train_acc']:.4f}, Val Acc: {rec['val_acc']:.4f} | {rec['images_per_sec']:.1f} img/s")
            if "fg_windows" in rec:
                print(f"Foreground-centred windows: {rec['fg_windows']} of {seen}")
            if "lr" in rec:
                print(f"Learning rate: {rec['lr']:.3e}")
            if "grad_norm_mean" in rec:
                print(f"Gradient norm (mean): {rec['grad_norm_mean']:.4g}, clipped steps: {rec['clipped_steps']}, "
                      f"skipped steps: {rec['skipped_steps']}")
            print("-------------------------------------------------------")
        if rec["val_dice"] > best_dice:
            best_dice, patience_counter = rec["val_dice"], 0
            saved_this_run = True       # (decided from rank 0's broadcast Dice: the same on every rank)
            if rank == 0:
                with ema_weights():                         # (--ema: the checkpoint holds the averaged weights)
                    torch.save(model.state_dict(), args.ckpt_path)
                print("Model saved!")
        else:
            patience_counter += 1
        if patience_counter >= args.patience:
            if rank == 0:
                print("Early stopping!")
            break
    # -------- final test evaluation (train_DC_focal.py:365-402, :452-467): best checkpoint, held-out split --------
    if world > 1:
        torch.distributed.barrier()                         # rank 0 has finished writing the checkpoint
    if args.test_eval and len(test_ds) > 0:
        if saved_this_run and os.path.exists(args.ckpt_path):
            model.load_state_dict(torch.load(args.ckpt_path, map_location=device, weights_only=True))
            ema_weights = contextlib.nullcontext            # (--ema: the checkpoint IS the averaged weights of the best epoch)
        elif rank == 0:
            # validation Dice never rose above 0: nothing was written by THIS run, and a file of that name left by an earlier
            # run (possibly another architecture) is not this run's result
            print(f"No checkpoint was written this run ({args.ckpt_path} not reloaded): evaluating the current weights")
        if not args.device_data:
            test_loader = DataLoader(test_ds, batch_size=args.batch, shuffle=False, num_workers=args.workers,
                                     pin_memory=pin)
        # every rank: same weights, same split
        with ema_weights():
            history.test = evaluate_test(model, test_loader, criterion, device, args.tta, args.batch, args.boundary,
                                         args.diff_maps if rank == 0 else None)
        if rank == 0:
            t = history.test
            print("========== Test Results ==========" + (f" (--tta {args.tta})" if args.tta != 1 else ""))
            print(f"Test Loss: {t['test_loss']:.4f}")
            print(f"Test Dice: {t['test_dice']:.4f}")
            print(f"Test Accuracy (pixel-wise): {t['test_acc']:.4f}")
            print(f"Precision: {t['precision']:.4f}, Recall: {t['recall']:.4f}, F1: {t['f1']:.4f}, "
                  f"Specificity: {t['specificity']:.4f}")
            print(f"Confusion matrix [[tn, fp], [fn, tp]]: {t['confusion']}")
            if "boundary" in t:
                b = t["boundary"]
                per_tol = ", ".join(f"nsd_{q} {b[f'nsd_{q}']:.4f}, bf_{q} {b[f'bf_{q}']:.4f}" for q in (1, 2, 3) if f"nsd_{q}" in b)
                print(f"Boundary (--boundary {b['R']}, pooled): HD95 {b['hd95']:.3f} px, ASSD {b['assd']:.3f} px, {per_tol}")
            if "diff_regions" in t:
                d = t["diff_regions"]
                print(f"Difference maps under {args.diff_maps}: regions yellow {d['yellow_blobs']}, red {d['red_blobs']}, green "
                      f"{d['green_blobs']}, black {d['black_blobs']}; missed droplets {d['missed_droplets']}, spurious "
                      f"{d['spurious_droplets']}")
    if args.calibrate_thresh is not None and len(val_ds) > 0:
        with ema_weights():                                 # the weights the test evaluation used
            history.calibration = calibrate_threshold(model, val_loader, args.calibrate_thresh, device, args.tta,
                                                        args.batch)         # every rank: same weights
        if rank == 0:
            c = history.calibration
            with_tta = f", --tta {args.tta}" if args.tta != 1 else ""
            print(f"Threshold calibration on the validation split (K = {c['K']}{with_tta}): pooled Dice {c['best_dice']:.4f} at "
                  f"threshold {c['best_dice_threshold']:.6g}; average precision {c['average_precision']:.4f}")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    gc.unfreeze()                   # (a caller that runs main() in-process gets its objects back under the collector)
    return history


if __name__ == "__main__":
    main()
