#!/usr/bin/env python3
"""Training throughput of train_DC_focal.py on N synthetic 1040 x 1388 PNG pairs (bench.synthetic_micrograph images, masks by
threshold), three arms (four with --crop), each in a fresh child process, bf16, batch 8:
    synthetic    --synthetic --synthetic_len N        (generated tiles: the loader is not the limit)
    device_data  --device_data                        (cache on the device, augmentation kernels per batch)
    cpu_loader   the host loader (SegmentationDataset + TrainAugment, --workers 4), capped with --steps
    crop         --device_data --crop S               (with --crop[=S]: images cached at native size, S x S random windows cut
                                                       and augmented per batch; S = 512 has the step shapes of device_data)
Prints the per-epoch training img/s of every arm and one JSON line with the mean from epoch 2 on.

    python tools/train_e2e.py [N] [--epochs E] [--cpu_steps S] [--crop[=S]] [--crop_scale LO HI] [--crop_fg P]
                              [--only ARM [--only ARM ...]]

--crop_scale / --crop_fg are passed through to every run of the crop arm (scale jitter and foreground-aware windows).

--only may be repeated, also with one arm twice (two runs of one arm in one job give the run-to-run spread): the second run
of an arm is reported as ARM_run2."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = ("synthetic", "device_data", "cpu_loader")
CROP_ARM = "crop"


def write_pairs(d, n):
    import numpy as np
    from PIL import Image

    import bench
    ind, md = os.path.join(d, "images"), os.path.join(d, "masks")
    os.makedirs(ind)
    os.makedirs(md)
    base = [bench.synthetic_micrograph(7 + i) for i in range(8)]
    for i in range(n):
        img = np.roll(base[i % 8], 53 * (i // 8), axis=1)
        Image.fromarray(img).save(os.path.join(ind, f"img_{i:04d}.png"), compress_level=1)
        Image.fromarray(((img[..., 0] > 110) * 255).astype(np.uint8)).save(os.path.join(md, f"img_{i:04d}.png"),
                                                                            compress_level=1)
    return ind, md


def run_arm(arm, n, ind, md, epochs, cpu_steps, d, crop=512, crop_flags=()):
    common = ["--dtype", "bf16", "--batch", "8", "--epochs", str(epochs), "--patience", str(epochs + 1), "--no_test_eval",
              "--ckpt_path", os.path.join(d, f"{arm}.pth")]
    if arm == "synthetic":
        extra = ["--synthetic", "--synthetic_len", str(n)]
    elif arm == "device_data":
        extra = ["--image_dir", ind, "--mask_dir", md, "--device_data"]
    elif arm == CROP_ARM:
        extra = ["--image_dir", ind, "--mask_dir", md, "--device_data", "--crop", str(crop), *crop_flags]
    else:
        extra = ["--image_dir", ind, "--mask_dir", md, "--steps", str(cpu_steps), "--workers", "4"]
    cmd = [sys.executable, os.path.join(ROOT, "train_DC_focal.py"), *common, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(f"--- {arm}: exit {r.returncode}\n" + "\n".join(l for l in r.stdout.splitlines() if "img/s" in l) + "\n")
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"arm {arm} failed (exit {r.returncode})")
    return [float(v) for v in re.findall(r"\|\s*([0-9.]+) img/s", r.stdout)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=400)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--cpu_steps", type=int, default=3)
    ap.add_argument("--crop", type=int, nargs="?", const=512, default=None, metavar="S",
                    help="also run the crop arm (train_DC_focal.py --device_data --crop S; 512 without S)")
    ap.add_argument("--crop_scale", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="crop arm: --crop_scale LO HI")
    ap.add_argument("--crop_fg", type=float, default=None, metavar="P", help="crop arm: --crop_fg P")
    ap.add_argument("--only", choices=ARMS + (CROP_ARM,), action="append")
    a = ap.parse_args()
    res = {"n_pairs": a.n, "epochs": a.epochs, "batch": 8, "dtype": "bf16", "cpu_loader_steps_per_epoch": a.cpu_steps}
    crop = 512 if a.crop is None else a.crop
    arms = a.only or (ARMS + ((CROP_ARM,) if a.crop is not None else ()))
    crop_flags = []
    if a.crop_scale is not None:
        crop_flags += ["--crop_scale", *(repr(v) for v in a.crop_scale)]
    if a.crop_fg is not None:
        crop_flags += ["--crop_fg", repr(a.crop_fg)]
    if CROP_ARM in arms:
        res["crop"] = crop
        res["crop_flags"] = crop_flags
    with tempfile.TemporaryDirectory() as d:
        ind, md = write_pairs(d, a.n)
        for j, arm in enumerate(arms):
            ips = run_arm(arm, a.n, ind, md, a.epochs, a.cpu_steps, d, crop, crop_flags)
            runs = list(arms[:j]).count(arm)
            key = arm if not runs else f"{arm}_run{runs + 1}"
            res[f"{key}_img_per_s_by_epoch"] = ips
            res[f"{key}_img_per_s"] = sum(ips[1:]) / max(1, len(ips[1:]))
    if "synthetic_img_per_s" in res and "device_data_img_per_s" in res:
        res["device_data_over_synthetic"] = res["device_data_img_per_s"] / res["synthetic_img_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
