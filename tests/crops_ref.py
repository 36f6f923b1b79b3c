"""Plain-loop restatement of the crop rule (utils/crops.py, csrc/crop.hip) and the fixtures its CPU and GPU tests share: one
output pixel at a time, no slicing, no np.rot90, no utils.tiling.fold."""
import numpy as np

S = 32
# larger than the crop, equal to it, one axis folded, a single pixel, both sides one past / well past the crop
SHAPES = [(40, 56), (32, 32), (20, 70), (1, 1), (33, 47)]


def fold_loop(i, dim):
    """reflect-101 by mirroring at the two border pixels until the coordinate lies inside."""
    if dim == 1:
        return 0
    while i < 0 or i >= dim:
        i = -i if i < 0 else 2 * (dim - 1) - i
    return i


def source_loop(y, x, n, p):
    """Output pixel (y, x) of rot90(vflip(hflip(win)), k) on an n x n window -> the window pixel it shows."""
    k = p["k"]
    if k == 0:
        fy, fx = y, x
    elif k == 1:                       # np.rot90(m)[y][x] = m[x][n - 1 - y]
        fy, fx = x, n - 1 - y
    elif k == 2:
        fy, fx = n - 1 - y, n - 1 - x
    else:                              # np.rot90(m, 3)[y][x] = m[n - 1 - x][y]
        fy, fx = n - 1 - x, y
    if p["vflip"]:
        fy = n - 1 - fy
    if p["hflip"]:
        fx = n - 1 - fx
    return fy, fx


def crop_sample_loops(img, mask, y0, x0, s, p):
    """One sample without elastic: (out [C, s, s] float32, mask [1, s, s] float32)."""
    h, w, c = img.shape
    out, om = np.empty((c, s, s), np.float32), np.empty((1, s, s), np.float32)
    beta_max = np.float32(p["beta"] * float(np.float32(int(img.max())) / np.float32(255.0)))
    for y in range(s):
        for x in range(s):
            wy, wx = source_loop(y, x, s, p)
            iy, ix = fold_loop(y0 + wy, h), fold_loop(x0 + wx, w)
            om[0, y, x] = np.float32(mask[iy, ix])
            v = img[iy, ix].astype(np.float32) / np.float32(255.0)               # (the pixel's channels at once)
            if p["bc"]:
                v = (np.float32(p["alpha"]) * v).astype(np.float32) + beta_max
                v = np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))
            out[:, y, x] = v
    return out, om


def images(channels=3, bright=True, seed=0):
    """One uint8 [h, w, channels] image and {0, 1} mask per entry of SHAPES.  bright: the four corner pixels are 255, so every
    window at an end origin holds the image's maximum (the window's maximum then IS the image's: the restatement of the
    resized path, augment_ref.augment_with_params, applies to the window unchanged).  Not bright: values up to 200 and one
    pixel of 231 in the bottom-left corner, outside the windows at y0 = 0 of an image taller than the crop."""
    r = np.random.default_rng(seed)
    imgs, masks = [], []
    for h, w in SHAPES:
        img = r.integers(0, 201, (h, w, channels), dtype=np.uint8)
        if bright:
            img[0, 0] = img[0, -1] = img[-1, 0] = img[-1, -1] = 255
        else:
            img[-1, 0] = 231
        imgs.append(img)
        masks.append((r.random((h, w)) < 0.3).astype(np.uint8))
    return imgs, masks


def end_origins(h, w, s=S):
    """The origins at 0 and at dim - s on either axis (one origin on an axis the crop covers)."""
    return [(y0, x0) for y0 in sorted({0, max(h - s, 0)}) for x0 in sorted({0, max(w - s, 0)})]


def params(hflip=False, vflip=False, k=0, bc=False, alpha=1.0, beta=0.0, elastic=False, field_seed=0):
    return dict(hflip=hflip, vflip=vflip, k=k, bc=bc, alpha=alpha, beta=beta, elastic=elastic, field_seed=field_seed)


def records(seed=1, bc_share=0.5):
    """Every image of SHAPES at each of its end origins with every k and both flips (5 images, 12 origins in all, 16
    geometric combinations each = 192 records), brightness / contrast on about half of them."""
    r = np.random.default_rng(seed)
    recs = []
    for i, (h, w) in enumerate(SHAPES):
        for y0, x0 in end_origins(h, w):
            for k in range(4):
                for hf in (False, True):
                    for vf in (False, True):
                        bc = bool(r.random() < bc_share)
                        recs.append(dict(img=i, y0=y0, x0=x0, params=params(
                            hf, vf, k, bc, 1.0 + r.uniform(-0.2, 0.2) if bc else 1.0, r.uniform(-0.2, 0.2) if bc else 0.0)))
    return recs


# ---- unetdc_crop_gather calls that must be refused ------------------------------------------------------------------------------
def _record(**kw):
    from unet_dc_segmentation_amd.crops import CROP_DTYPE
    r = np.zeros(1, CROP_DTYPE)
    r["h"], r["w"], r["field"], r["alpha"] = 40, 56, -1, 1.0
    for k, v in kw.items():
        r[k] = v
    return r


REFUSED = {
    "size not a multiple of 16": (dict(), dict(S=40)),
    "size below 16": (dict(), dict(S=0)),
    "size above 1024": (dict(), dict(S=1040)),
    "no channels": (dict(), dict(c=0)),
    "five channels": (dict(), dict(c=5)),
    "height 0": (dict(h=0), dict()),
    "width above 16384": (dict(w=16385), dict()),
    "y0 negative": (dict(y0=-1), dict()),
    "y0 past h - S": (dict(y0=9), dict()),
    "x0 past w - S": (dict(x0=25), dict()),
    "y0 on a folded axis": (dict(h=20, y0=1), dict()),
    "image leaves its buffer": (dict(img_off=1), dict()),
    "image offset negative": (dict(img_off=-8), dict()),
    "mask leaves its buffer": (dict(mask_off=1), dict()),
    "k = 4": (dict(k=4), dict()),
    "k negative": (dict(k=-1), dict()),
    "unknown flag": (dict(flags=8), dict()),
    "field slot = nfields": (dict(field=0), dict()),
    "field slot below -1": (dict(field=-2), dict()),
    "field without fields": (dict(field=0), dict(nfields=1)),
    "null images": (dict(), dict(images=None)),
    "null masks": (dict(), dict(masks=None)),
    "null records": (dict(), dict(records=None)),
    "null image output": (dict(), dict(out_img=None)),
    "null mask output": (dict(), dict(out_mask=None)),
}


def refused_call(lib, name, ptrs):
    """One refused unetdc_crop_gather: a 40 x 56 x 3 image that exactly fills its buffers, S = 32, one record, with the
    changes of REFUSED[name].  ptrs: dict(images, masks, out_img, out_mask) addresses."""
    rec_kw, call_kw = REFUSED[name]
    rec = _record(**rec_kw)
    a = dict(ptrs, S=S, c=3, records=rec.ctypes.data, nfields=0, fields=None)
    a.update(call_kw)
    return lib.unetdc_crop_gather(a["images"], 40 * 56 * a["c"] if a["c"] > 0 else 0, a["masks"], 40 * 56, a["c"], a["S"],
                                  a["records"], 1, a["fields"], a["nfields"], a["out_img"], a["out_mask"], None)
