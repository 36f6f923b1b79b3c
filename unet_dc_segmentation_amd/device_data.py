"""Device-resident training data: every image is decoded and preprocessed ONCE (rolling ball, resize, /255 on the HIP device,
``preprocess.preprocess_device``) into a cache on the device, and each training batch is augmented there by the kernels of
csrc/augment.hip.  The CPU path (``utils.data_loader.SegmentationDataset`` + ``TrainAugment``) repeats decode, rolling ball,
resize and augmentation for every sample of every epoch on the host, which holds real-data training to a few images/s.

Batches have the layout of a default-collated ``SegmentationDataset``: ``(images [B, C, S, S] float32, masks [B, 1, S, S]
float32, [orig_h tensor, orig_w tensor], [file names])``, already on the device.  The training augmentation draws a
counter-based random stream (``augment.draw_params``, keyed by ``(seed, epoch, index)``), not TrainAugment's.

``DeviceNativeCache`` / ``DeviceCropTrainLoader`` / ``DeviceCropEvalLoader`` (``--crop``) keep the images
at their own size instead and cut S x S windows per batch (csrc/crop.hip): training at native resolution.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import augment
from .preprocess import preprocess_device, preprocess_device_u8


def _decode_image(image_path, intensity):
    """uint8 RGB as before (a deep file clipped at 255, reported once), or with a window (utils.intensity_window.WindowSpec)
    the uint16 image of decode_deep, which _windowed() takes to 8 bits on the device."""
    from utils import intensity_window as iw
    return iw.decode_rgb_clipped(image_path) if intensity is None else iw.decode_deep(image_path, intensity.page)


def _windowed(img, intensity, device):
    """Decoded image -> what the preprocessing takes: the host array as it is, or with a window the [h, w, 3] uint8 DEVICE
    tensor of window.deep_to_u8_device."""
    if intensity is None:
        return img
    from .window import deep_to_u8_device
    return deep_to_u8_device(img, intensity, device)[0]


def _decode_pair(image_path, mask_path, size, intensity=None):
    """(uint8 RGB image, its (h, w), uint8 {0, 1} mask nearest-resized to size x size) -- SegmentationDataset's host steps."""
    from utils.data_loader import resize_image
    img = _decode_image(image_path, intensity)
    if mask_path is None:                                         # mask_polygons: the mask comes from the rasteriser
        return img, img.shape[:2], None
    mask = (np.array(Image.open(mask_path).convert("L")) > 0).astype(np.uint8)
    return img, img.shape[:2], resize_image(mask, size, nearest=True)


def _polygon_masks(mask_polygons, names, hws, device):
    """mask_polygons ({image name: packed record of utils.polygon_masks.pack}) -> per image the uint8 {0, 1} DEVICE mask
    [h, w] at the image's own size: labels > 0 of polygons.rasterize_batch, one batch per call."""
    from .polygons import rasterize_batch
    missing = [n for n in names if n not in mask_polygons]
    if missing:
        raise ValueError(f"mask_polygons: no polygons for {missing[0]}")
    recs = rasterize_batch([mask_polygons[n] for n in names], hws, compact=False, device=device)
    return [(r["labels"] > 0).to(torch.uint8) for r in recs]


class DeviceImageCache:
    """Preprocessed images [N, 3, size, size] float32 and masks [N, size, size] uint8 on `device`, bit-identical to
    ``SegmentationDataset(image_dir, mask_dir, names, mask_names, size=size, radius=radius)[i][:2]`` before its transform;
    ``img_max[i]`` is the image's maximum (the ``img.max()`` of the brightness / contrast step).  Files are decoded on a small
    thread pool (PIL releases the GIL while it inflates), in windows so that at most a few dozen decoded images are held.
    mask_polygons ({image name: packed polygons}): the mask is the rasterised annotation (labels > 0 at the image's own size,
    filled on the device) instead of a file of mask_dir, and takes the same nearest resize from there."""

    def __init__(self, image_dir, mask_dir, names, size=512, radius=50, device="cuda", mask_names=None, workers=None,
                 mask_polygons=None, intensity=None):
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
                jobs = [ex.submit(_decode_pair, os.path.join(image_dir, self.names[i]),
                                  None if mask_polygons is not None else os.path.join(mask_dir, mask_names[i]), size, intensity)
                        for i in range(w0, min(n, w0 + window))]
                done = [job.result() for job in jobs]
                if mask_polygons is not None:
                    from utils.data_loader import resize_image
                    filled = _polygon_masks(mask_polygons, self.names[w0:w0 + len(done)], [d[1] for d in done], device)
                    done = [(img, hw, resize_image(m.cpu().numpy(), size, nearest=True)) for (img, hw, _), m in zip(done, filled)]
                for i, (img, hw, mask) in enumerate(done, start=w0):
                    self.orig_sizes.append(tuple(int(v) for v in hw))
                    if intensity is None:
                        self.images[i].copy_(preprocess_device(img, radius, size, device))
                    else:                                         # deep image: windowed to 8 bits on the device first
                        self.images[i].copy_(preprocess_device_u8(_windowed(img, intensity, device), radius, size))
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


# ---- training at native resolution: images cached at their own size, random crops cut on the device ----
def _decode_native(image_path, mask_path, intensity=None):
    """(uint8 RGB image [h, w, 3], uint8 {0, 1} mask [h, w] at the image's own size: grey > 0, not resized)."""
    img = _decode_image(image_path, intensity)
    if mask_path is None:                                         # mask_polygons: the mask comes from the rasteriser
        return img, None
    mask = (np.array(Image.open(mask_path).convert("L")) > 0).astype(np.uint8)
    if mask.shape != img.shape[:2]:
        raise ValueError(f"{mask_path}: the mask is {mask.shape[0]} x {mask.shape[1]}, its image {img.shape[0]} x {img.shape[1]}")
    return img, mask


class DeviceNativeCache:
    """Rolling-ball-corrected images at their OWN size, HWC uint8, back to back in one flat device buffer (``images``), and
    their {0, 1} masks in another (``masks``): 4 bytes per pixel against the 13 of a float32 cache.  On the host: per-image
    byte offsets (``img_off``, ``mask_off``), ``sizes`` [(h, w)] and ``img_max`` (float32(max) / float32(255) of the corrected
    image as a double: the maximum of the brightness / contrast step).  Images may differ in size.  Decoding runs on the thread
    pool of DeviceImageCache; the rolling ball on the device (above radius 128 the host operator, as preprocess_device).
    Every file is opened twice: once for its header alone, so that the memory check comes before any allocation or decode,
    and once to decode it (a second pass over the directory, which a network file system will notice).

    keep_foreground: also keep, on the HOST, ``foreground[i] = np.flatnonzero(mask).astype(np.int32)`` of every image, taken
    from the mask as it is decoded (the mask itself is still not kept): the pixels utils.crops.draw_crop_fg places a
    foreground-aware window on.  4 bytes per foreground pixel: about 0.6 MB for a 1040 x 1388 image that is 10 % covered
    (144 000 pixels), 5.8 MB for a fully covered one.

    mask_polygons ({image name: packed polygons}): the mask is the rasterised annotation (labels > 0, filled on the device at the
    image's size) instead of a file of mask_dir; it never visits the host unless keep_foreground asks for its pixels."""
    channels = 3

    def __init__(self, image_dir, mask_dir, names, radius=50, device="cuda", mask_names=None, workers=None,
                 keep_foreground=False, mask_polygons=None, intensity=None):
        from .preprocess import MAX_ELEMENT, _upload, rolling_ball_device
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("DeviceNativeCache keeps the images on the HIP device: device must be a cuda device")
        self.names = list(names)
        mask_names = self.names if mask_names is None else list(mask_names)
        if len(mask_names) != len(self.names):
            raise ValueError("DeviceNativeCache: one mask per image")
        n, self.device = len(self.names), device
        self.sizes = []
        for name in self.names:                                   # (the header only: PIL decodes nothing here)
            with Image.open(os.path.join(image_dir, name)) as im:
                self.sizes.append((int(im.size[1]), int(im.size[0])))
        pixels = [h * w for h, w in self.sizes]
        self.mask_off = [int(v) for v in np.concatenate([[0], np.cumsum(pixels, dtype=np.int64)])[:n]]
        self.img_off = [self.channels * v for v in self.mask_off]
        need = (self.channels + 1) * sum(pixels)
        free, total = torch.cuda.mem_get_info(device)
        if need > free:
            raise MemoryError(f"DeviceNativeCache: {n} images at their own size need {need / 2**30:.2f} GiB on {device}, "
                              f"{free / 2**30:.2f} GiB of {total / 2**30:.2f} GiB are free; train without --crop or on "
                              f"fewer images")
        self.images = torch.empty(self.channels * sum(pixels), dtype=torch.uint8, device=device)
        self.masks = torch.empty(sum(pixels), dtype=torch.uint8, device=device)
        self.img_max = np.zeros(n)
        self.foreground = [None] * n if keep_foreground else None
        workers = workers or min(8, os.cpu_count() or 1)
        window = 4 * workers
        with ThreadPoolExecutor(max_workers=workers) as ex:
            for w0 in range(0, n, window):
                jobs = [ex.submit(_decode_native, os.path.join(image_dir, self.names[i]),
                                  None if mask_polygons is not None else os.path.join(mask_dir, mask_names[i]), intensity)
                        for i in range(w0, min(n, w0 + window))]
                done = [job.result() for job in jobs]
                if mask_polygons is not None:
                    filled = _polygon_masks(mask_polygons, self.names[w0:w0 + len(done)], [d[0].shape[:2] for d in done], device)
                    done = [(img, m) for (img, _), m in zip(done, filled)]
                for i, (img, mask) in enumerate(done, start=w0):
                    if img.shape[:2] != self.sizes[i]:
                        raise ValueError(f"{self.names[i]}: decoded to {img.shape[:2]}, its header says {self.sizes[i]}")
                    img = _windowed(img, intensity, device)           # deep image: windowed to 8 bits on the device first
                    if int(radius) > MAX_ELEMENT:
                        from utils.data_loader import rolling_ball_correction_rgb
                        host = img.cpu().numpy() if torch.is_tensor(img) else img
                        rgb = _upload(rolling_ball_correction_rgb(host, int(radius)), device)
                    else:
                        rgb = rolling_ball_device(img if torch.is_tensor(img) else _upload(img, device), radius)
                    self.image(i).copy_(rgb)
                    self.mask(i).copy_(mask if torch.is_tensor(mask) else torch.from_numpy(mask))
                    if keep_foreground:
                        self.foreground[i] = np.flatnonzero(mask.cpu().numpy() if torch.is_tensor(mask) else mask).astype(np.int32)
                    self.img_max[i] = float(np.float32(int(rgb.max())) / np.float32(255.0))       # (once, at build)
        self.orig_sizes = self.sizes

    def __len__(self):
        return len(self.names)

    def image(self, i):
        """View of image i, [h, w, 3] uint8."""
        h, w = self.sizes[i]
        return self.images[self.img_off[i]:self.img_off[i] + h * w * self.channels].view(h, w, self.channels)

    def mask(self, i):
        h, w = self.sizes[i]
        return self.masks[self.mask_off[i]:self.mask_off[i] + h * w].view(h, w)

    def _meta(self, idx):
        return ([torch.tensor([self.sizes[i][0] for i in idx]), torch.tensor([self.sizes[i][1] for i in idx])],
                [self.names[i] for i in idx])

    def gather(self, S, idx, origins, params, fields=None, ts=None):
        """One unetdc_crop_gather over the windows `origins` of the images `idx` with the augment.draw_params dicts `params`.
        ts: the sides of the source windows at `origins`, resampled to S x S by one unetdc_crop_gather_scaled instead."""
        from . import crops
        args = (params, [self.img_off[i] for i in idx], [self.mask_off[i] for i in idx], [self.sizes[i] for i in idx], origins,
                [self.img_max[i] for i in idx])
        if ts is None:
            return crops.crop_gather(self.images, self.masks, self.channels, S, crops.pack_crops(*args)[0], fields)
        return crops.crop_gather_scaled(self.images, self.masks, self.channels, S, crops.pack_crops_scaled(*args, ts)[0], fields)


class DeviceCropTrainLoader:
    """Shuffled, augmented S x S crops of a DeviceNativeCache, no drop_last: N images give N * R samples per epoch
    (R = crops_per_image).  Epoch e visits them in the order np.random.default_rng([seed, e]).permutation(N * R); local sample
    number j is crop rep = j % R of cached image i = j // R and draws as sample q = ids[i] * R + rep of the whole training
    split: its window from utils.crops.draw_crop(seed, e, q, h, w, S), its augmentation from augment.draw_params(seed, e, q).
    Per batch: at most one elastic-field launch (S x S) and one unetdc_crop_gather, parameters by value; nothing waits on the
    device.

    scale = (LO, HI) and / or p_fg > 0 (--crop_scale, --crop_fg): the window comes from utils.crops.draw_crop_fg(seed, e, q,
    h, w, S, scale, p_fg, cache.foreground[i]) instead -- a source side T of utils.crops.t_range(S, scale) (T = S without
    scale), with probability p_fg placed on a foreground pixel of its image (the cache must have been built with
    keep_foreground=True) -- and the batch from one unetdc_crop_gather_scaled, which resamples every T x T window to S x S.
    ``fg_windows`` counts the windows of the epoch being served that took the foreground branch.  With both off nothing
    changes: draw_crop and unetdc_crop_gather."""

    def __init__(self, cache, batch_size, S, seed=0, ids=None, crops_per_image=1, sigma=augment.ELASTIC_SIGMA,
                 alpha=augment.ELASTIC_ALPHA, scale=None, p_fg=0.0):
        from utils.crops import check_crop, check_scale
        self.dataset, self.batch_size, self.S, self.seed = cache, int(batch_size), check_crop(S), int(seed)
        self.ids = list(range(len(cache))) if ids is None else [int(i) for i in ids]
        if len(self.ids) != len(cache):
            raise ValueError("DeviceCropTrainLoader: one global index per cached image")
        self.R = int(crops_per_image)
        if self.R < 1:
            raise ValueError("DeviceCropTrainLoader: crops_per_image must be at least 1")
        self.sigma, self.alpha = float(sigma), float(alpha)
        self.scale, self.p_fg = None if scale is None else check_scale(scale), float(p_fg)
        if not 0.0 <= self.p_fg <= 1.0:
            raise ValueError(f"DeviceCropTrainLoader: p_fg {self.p_fg} outside [0, 1]")
        if self.p_fg > 0.0 and getattr(cache, "foreground", None) is None:
            raise ValueError("DeviceCropTrainLoader: p_fg > 0 needs a cache built with keep_foreground=True")
        self.scaled = self.scale is not None or self.p_fg > 0.0
        self.fg_windows = 0
        self.epoch = 0
        s = self.S
        self._fields = torch.empty(self.batch_size, 2, s, s, dtype=torch.float32, device=cache.device)
        self._ws = torch.empty(augment.fields_workspace_bytes(self.batch_size, s, s, self.sigma), dtype=torch.uint8,
                               device=cache.device)

    @property
    def samples(self):
        return len(self.dataset) * self.R

    def __len__(self):
        return (self.samples + self.batch_size - 1) // self.batch_size

    def records(self, epoch, js):
        """(cache indices, origins, source sides, draw_params dicts, took-the-foreground-branch flags) of the local sample
        numbers `js` in epoch `epoch`.  Without scale and p_fg the sides are None and no flag is set."""
        from utils import crops
        c = self.dataset
        idx = [int(j) // self.R for j in js]
        qs = [self.ids[i] * self.R + int(j) % self.R for i, j in zip(idx, js)]
        params = [augment.draw_params(self.seed, epoch, q) for q in qs]
        if not self.scaled:
            origins = [crops.draw_crop(self.seed, epoch, q, *c.sizes[i], self.S) for i, q in zip(idx, qs)]
            return idx, origins, None, params, [False] * len(idx)
        draws = [crops.draw_crop_fg_branch(self.seed, epoch, q, *c.sizes[i], self.S, self.scale, self.p_fg,
                                           c.foreground[i] if self.p_fg > 0.0 else None) for i, q in zip(idx, qs)]
        return (idx, [(y0, x0) for y0, x0, _, _ in draws], [t for _, _, t, _ in draws], params, [fg for _, _, _, fg in draws])

    def batch(self, epoch, js):
        """The augmented batch of local sample numbers `js` in epoch `epoch`."""
        c = self.dataset
        idx, origins, ts, params, took = self.records(epoch, js)
        self.fg_windows += sum(took)
        seeds = np.asarray([p["field_seed"] for p in params if p["elastic"]], dtype=np.uint32)
        fields = None
        if len(seeds):
            fields = augment.elastic_fields(seeds, self.S, self.S, self.sigma, self.alpha, out=self._fields,
                                            workspace=self._ws)[:len(seeds)]
        images, masks = c.gather(self.S, idx, origins, params, fields, ts)
        sizes, names = c._meta(idx)
        return images, masks, sizes, names

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        self.fg_windows = 0
        perm = np.random.default_rng([self.seed, epoch]).permutation(self.samples)
        for b0 in range(0, len(perm), self.batch_size):
            yield self.batch(epoch, perm[b0:b0 + self.batch_size])


class DeviceCropEvalLoader:
    """The utils.crops.eval_plan windows of every cached image in order (image by image, row-major), batch_size at a time,
    through unetdc_crop_gather with identity records: validation and test at the scale the crops train at.  Where the evenly
    spread windows of an image overlap, a pixel is counted by each window that covers it."""

    def __init__(self, cache, batch_size, S):
        from utils.crops import check_crop, eval_plan
        self.dataset, self.batch_size, self.S = cache, int(batch_size), check_crop(S)
        self.windows = [(i, y0, x0) for i, (h, w) in enumerate(cache.sizes) for y0, x0 in eval_plan(h, w, self.S)]

    def __len__(self):
        return (len(self.windows) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        from .crops import IDENTITY
        c = self.dataset
        for b0 in range(0, len(self.windows), self.batch_size):
            win = self.windows[b0:b0 + self.batch_size]
            idx = [i for i, _, _ in win]
            images, masks = c.gather(self.S, idx, [(y0, x0) for _, y0, x0 in win], [IDENTITY] * len(win))
            sizes, names = c._meta(idx)
            yield images, masks, sizes, names
