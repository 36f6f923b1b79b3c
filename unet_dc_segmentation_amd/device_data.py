"""Device-resident training data: every image is decoded and preprocessed ONCE (rolling ball, resize, /255 on the HIP device,
``preprocess.preprocess_device``) into a cache on the device, and each training batch is augmented there by the kernels of
csrc/augment.hip.  The CPU path (``utils.data_loader.SegmentationDataset`` + ``TrainAugment``) repeats decode, rolling ball,
resize and augmentation for every sample of every epoch on the host, which holds real-data training to a few images/s.

Batches have the layout of a default-collated ``SegmentationDataset``: ``(images [B, C, S, S] float32, masks [B, 1, S, S]
float32, [orig_h tensor, orig_w tensor], [file names])``, already on the device.  The training augmentation draws a
counter-based random stream (``augment.draw_params``, keyed by ``(seed, epoch, index)``), not TrainAugment's.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import augment
from .preprocess import preprocess_device


def _decode_pair(image_path, mask_path, size):
    """(uint8 RGB image, its (h, w), uint8 {0, 1} mask nearest-resized to size x size) -- SegmentationDataset's host steps."""
    from utils.data_loader import resize_image
    img = np.array(Image.open(image_path).convert("RGB"))
    mask = (np.array(Image.open(mask_path).convert("L")) > 0).astype(np.uint8)
    return img, img.shape[:2], resize_image(mask, size, nearest=True)


class DeviceImageCache:
    """Preprocessed images [N, 3, size, size] float32 and masks [N, size, size] uint8 on `device`, bit-identical to
    ``SegmentationDataset(image_dir, mask_dir, names, mask_names, size=size, radius=radius)[i][:2]`` before its transform;
    ``img_max[i]`` is the image's maximum (the ``img.max()`` of the brightness / contrast step).  Files are decoded on a small
    thread pool (PIL releases the GIL while it inflates), in windows so that at most a few dozen decoded images are held."""

    def __init__(self, image_dir, mask_dir, names, size=512, radius=50, device="cuda", mask_names=None, workers=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("DeviceImageCache keeps the images on the HIP device: device must be a cuda device")
        self.names = list(names)
        mask_names = self.names if mask_names is None else list(mask_names)
        if len(mask_names) != len(self.names):
            raise ValueError("DeviceImageCache: one mask per image")
        n, self.size, self.device = len(self.names), int(size), device
        need = n * (3 * size * size * 4 + size * size)
        free, total = torch.cuda.mem_get_info(device)
        if need > free:
            raise MemoryError(f"DeviceImageCache: {n} images at {size} x {size} need {need / 2**30:.2f} GiB on {device}, "
                              f"{free / 2**30:.2f} GiB of {total / 2**30:.2f} GiB are free; train without --device_data "
                              f"(the host loader) or with a smaller --img_size")
        self.images = torch.empty(n, 3, size, size, dtype=torch.float32, device=device)
        self.masks = torch.empty(n, size, size, dtype=torch.uint8, device=device)
        self.orig_sizes = []
        workers = workers or min(8, os.cpu_count() or 1)
        window = 4 * workers
        with ThreadPoolExecutor(max_workers=workers) as ex:
            for w0 in range(0, n, window):
                jobs = [ex.submit(_decode_pair, os.path.join(image_dir, self.names[i]), os.path.join(mask_dir, mask_names[i]),
                                  size) for i in range(w0, min(n, w0 + window))]
                for i, job in enumerate(jobs, start=w0):
                    img, hw, mask = job.result()
                    self.orig_sizes.append(tuple(int(v) for v in hw))
                    self.images[i].copy_(preprocess_device(img, radius, size, device))
                    self.masks[i].copy_(torch.from_numpy(mask))
        self.img_max = self.images.amax(dim=(1, 2, 3)).double().cpu().numpy() if n else np.zeros(0)   # (once, at build)

    def __len__(self):
        return len(self.names)

    def _meta(self, idx):
        return ([torch.tensor([self.orig_sizes[i][0] for i in idx]), torch.tensor([self.orig_sizes[i][1] for i in idx])],
                [self.names[i] for i in idx])


class DeviceEvalLoader:
    """Batches of the cache in order (a plain gather: the images are views of the cache), like
    ``DataLoader(SegmentationDataset(..., transform=None), batch_size, shuffle=False)``."""

    def __init__(self, cache, batch_size):
        self.dataset, self.batch_size = cache, int(batch_size)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        c = self.dataset
        for b0 in range(0, len(c), self.batch_size):
            b1 = min(len(c), b0 + self.batch_size)
            sizes, names = c._meta(range(b0, b1))
            yield c.images[b0:b1], c.masks[b0:b1].unsqueeze(1).float(), sizes, names


class DeviceTrainLoader:
    """Shuffled, augmented batches of the cache, no drop_last.  Epoch e (the e-th iteration of the loader) visits the cache
    in the order np.random.default_rng([seed, e]).permutation(N); sample i of the cache draws its augmentation from
    ``augment.draw_params(seed, e, ids[i])``, where ``ids`` are the samples' indices in the whole training split (a data-
    parallel rank caches only its shard), so the stream does not depend on batch size, world size or worker count.  Per
    batch: at most one elastic-field launch (for the samples that draw it) and one gather launch, parameters passed by value;
    nothing waits on the device."""

    def __init__(self, cache, batch_size, seed=0, ids=None, sigma=augment.ELASTIC_SIGMA, alpha=augment.ELASTIC_ALPHA):
        self.dataset, self.batch_size, self.seed = cache, int(batch_size), int(seed)
        self.ids = list(range(len(cache))) if ids is None else [int(i) for i in ids]
        if len(self.ids) != len(cache):
            raise ValueError("DeviceTrainLoader: one global index per cached sample")
        self.sigma, self.alpha = float(sigma), float(alpha)
        self.epoch = 0
        s = cache.size
        self._fields = torch.empty(self.batch_size, 2, s, s, dtype=torch.float32, device=cache.device)
        self._ws = torch.empty(augment.fields_workspace_bytes(self.batch_size, s, s, self.sigma), dtype=torch.uint8,
                               device=cache.device)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def batch(self, epoch, idx):
        """The augmented batch of cache samples `idx` in epoch `epoch`."""
        c = self.dataset
        params = [augment.draw_params(self.seed, epoch, self.ids[i]) for i in idx]
        rec, seeds = augment.pack_params(params, idx, c.img_max[idx])
        fields = None
        if len(seeds):
            fields = augment.elastic_fields(seeds, c.size, c.size, self.sigma, self.alpha, out=self._fields,
                                            workspace=self._ws)
        images, masks = augment.augment_gather(c.images, c.masks, rec, fields)
        sizes, names = c._meta(idx)
        return images, masks, sizes, names

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        perm = np.random.default_rng([self.seed, epoch]).permutation(len(self.dataset))
        for b0 in range(0, len(perm), self.batch_size):
            yield self.batch(epoch, perm[b0:b0 + self.batch_size])
