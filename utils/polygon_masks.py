"""Polygon annotations back into label maps: exact even-odd fill at pixel centres, the inverse of
utils/droplet_outlines.py.

Pixel (r, c) is the square [c, c + 1] x [r, r + 1], y down.  A vertex from a file is a float; it is quantised ONCE,
q = rint(v * 256) (half to even), and everything after that is integer.  The centre of pixel (r, c) is (256 c + 128,
256 r + 128).  A pixel is inside a *polygon* (one or more rings: an outer ring and its holes, or one COCO part) iff an odd
number of the polygon's edges (x0, y0) -> (x1, y1), over all its rings, have (y0 <= Y) != (y1 <= Y) and, ordered so that
y0 < y1, (X - x0) (y1 - y0) > (Y - y0) (x1 - x0).  Per row that is: an edge with y0 <= Y < y1 toggles the parity from column
k = floor(((Y - y0) (x1 - x0) + (x0 - 128) (y1 - y0)) / (256 (y1 - y0))) + 1 on.  A *feature* is one or more polygons with
one label; a pixel gets the largest label among the polygons that contain it.

``rasterize_numpy`` is the host path of what ``unetdc_polygon_fill`` computes on the device, and the yardstick of its tests.
No torch import.
"""
import json
import math
import os

import numpy as np

SUB = 256                         # sub-pixels per pixel
HALF = SUB // 2
MAX_COORD = 1 << 20               # pixels; a vertex beyond is refused
MAX_LABEL = 2 ** 31 - 1
MAX_SIDE = 16384


class PolygonError(ValueError):
    pass


# ---- readers ---------------------------------------------------------------------------------------------------------------------

def _ring(pts, where):
    """A ring from a file -> float64 [n, 2], its closing duplicate dropped."""
    try:
        a = np.asarray(pts, dtype=np.float64)
    except (TypeError, ValueError):
        raise PolygonError(f"{where}: a ring is not a list of [x, y] numbers") from None
    if a.ndim != 2 or a.shape[1] < 2:
        raise PolygonError(f"{where}: a ring is not a list of [x, y] numbers")
    a = a[:, :2]
    if len(a) >= 2 and np.array_equal(a[0], a[-1]):
        a = a[:-1]
    return a


def _rings(raw, wheres, depth):
    """Every ring of a file -> float64 [n, 2] arrays, closing duplicates dropped.  raw: the rings as the JSON parser left them,
    lists of [x, y] (depth 2) or flat [x0, y0, x1, ...] lists (depth 1); wheres: what to call each in a refusal.  ONE conversion
    for the file where every vertex is a pair of numbers (a conversion per ring costs more than parsing the text); anything else
    goes ring by ring through _ring, which says what is wrong."""
    from itertools import chain
    try:
        lens = [len(r) for r in raw]
        it = chain.from_iterable(raw)
        flat = np.fromiter(chain.from_iterable(it) if depth == 2 else it, dtype=np.float64)
        if depth == 1:
            lens = [n // 2 if n % 2 == 0 else -1 for n in lens]
        if min(lens, default=0) < 0 or flat.size != 2 * sum(lens):
            raise ValueError
    except (TypeError, ValueError):
        return [_ring(r if depth == 2 else np.asarray(r, dtype=np.float64).reshape(-1, 2), w) for r, w in zip(raw, wheres)]
    pts = flat.reshape(-1, 2)
    n = np.asarray(lens, dtype=np.int64)
    end = np.cumsum(n)
    first = end - n
    closed = np.zeros(len(n), bool)
    some = n >= 2
    closed[some] = (pts[first[some]] == pts[end[some] - 1]).all(axis=1)
    return [pts[a:b] for a, b in zip(first.tolist(), (end - closed).tolist())]


def _int_label(v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (math.inf, -math.inf) or int(v) != v:
        return None
    return int(v) if 1 <= int(v) <= MAX_LABEL else None


def _number(features):
    """The label rule: the labels the file carries if every feature has a positive integer of its own, else 1..F in file order."""
    given = [f["label"] for f in features]
    if not (all(g is not None for g in given) and len(set(given)) == len(given)):
        for i, f in enumerate(features):
            f["label"] = i + 1
    return features


def features_of_geojson(doc, name="geojson"):
    """A parsed GeoJSON FeatureCollection (or one Feature, or a bare geometry) -> features: a list of {"label": int,
    "polygons": [[ring, ...], ...]}, every ring a float64 [n, 2] array (outer ring first, then its holes)."""
    if doc.get("type") == "FeatureCollection":
        items = doc.get("features", [])
    elif doc.get("type") == "Feature":
        items = [doc]
    else:
        items = [{"type": "Feature", "properties": {}, "geometry": doc}]
    feats, raw, wheres = [], [], []
    for i, f in enumerate(items):
        where = f"{name}: feature {i}"
        g = f.get("geometry") or {}
        t = g.get("type")
        if t == "Polygon":
            polys = [g.get("coordinates", [])]
        elif t == "MultiPolygon":
            polys = g.get("coordinates", [])
        else:
            raise PolygonError(f"{where}: geometry type {t!r} (only Polygon and MultiPolygon can be filled)")
        polys = [poly for poly in polys if len(poly)]
        feats.append({"label": _int_label((f.get("properties") or {}).get("label")), "polygons": [len(poly) for poly in polys]})
        for poly in polys:
            raw += poly
            wheres += [where] * len(poly)
    rings, at = _rings(raw, wheres, 2), 0
    for f in feats:                                           # the rings back to their polygons, in file order
        counts, f["polygons"] = f["polygons"], []
        for n in counts:
            f["polygons"].append(rings[at:at + n])
            at += n
    return _number(feats)


def read_geojson(path):
    with open(path) as fh:
        return features_of_geojson(json.load(fh), str(path))


def images_of_coco(doc, name="coco"):
    """A parsed COCO file -> {file stem: (features, (h, w))}; every part of a segmentation is a polygon of one ring."""
    by_id, out = {}, {}
    for im in doc.get("images", []):
        stem = os.path.splitext(os.path.basename(str(im["file_name"])))[0]
        if stem in out:
            raise PolygonError(f"{name}: two images with the stem {stem!r}")
        out[stem] = ([], (int(im["height"]), int(im["width"])))
        by_id[im["id"]] = stem
    raw, wheres, owners = [], [], []
    for i, a in enumerate(doc.get("annotations", [])):
        where = f"{name}: annotation {a.get('id', i)}"
        if a.get("image_id") not in by_id:
            raise PolygonError(f"{where}: image_id {a.get('image_id')!r} is not listed under images")
        seg = a.get("segmentation")
        if isinstance(seg, dict):
            raise PolygonError(f"{where}: an RLE segmentation{' (iscrowd: 1)' if a.get('iscrowd') else ''} (only polygon lists can be filled)")
        if not isinstance(seg, list):
            raise PolygonError(f"{where}: no polygon segmentation")
        if any(not isinstance(part, list) or len(part) % 2 or (part and isinstance(part[0], list)) for part in seg):
            raise PolygonError(f"{where}: a segmentation part is not a flat [x0, y0, x1, y1, ...] list")
        feat = {"label": _int_label(a.get("label")), "polygons": []}
        out[by_id[a["image_id"]]][0].append(feat)
        raw += seg
        wheres += [where] * len(seg)
        owners += [feat] * len(seg)
    for feat, ring in zip(owners, _rings(raw, wheres, 1)):
        feat["polygons"].append([ring])
    for feats, _ in out.values():
        _number(feats)
    return out


def read_coco(path):
    with open(path) as fh:
        return images_of_coco(json.load(fh), str(path))


# ---- packing ---------------------------------------------------------------------------------------------------------------------

def quantise(v):
    """float vertices -> int32 sub-pixel coordinates; NaN, inf and |v| > 2^20 pixels are refused."""
    v = np.asarray(v, dtype=np.float64)
    if not np.isfinite(v).all():
        raise PolygonError("a vertex is NaN or infinite")
    if v.size and np.abs(v).max() > MAX_COORD:
        raise PolygonError(f"a vertex lies beyond 2^20 pixels ({np.abs(v).max()})")
    return np.rint(v * SUB).astype(np.int32)


def pack(features):
    """features -> the record the rasterisers read: verts int32 [V, 2] (x, y in sub-pixels), ring_first int32 [R + 1] (ring j
    owns verts[ring_first[j] : ring_first[j + 1]]), poly_first_ring int32 [P + 1], poly_label int32 [P]."""
    rings, owner, poly_first, labels = [], [], [0], []
    for i, f in enumerate(features):
        k = f["label"]
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_LABEL:
            raise PolygonError(f"feature {i}: label {k!r} is not an integer in 1..2^31 - 1")
        for poly in f["polygons"]:
            if not len(poly):
                continue
            rings += [np.asarray(ring, dtype=np.float64).reshape(-1, 2) for ring in poly]
            owner += [i] * len(poly)
            poly_first.append(len(rings))
            labels.append(int(k))
    lens = np.asarray([len(r) for r in rings], dtype=np.int64)
    if len(lens) and lens.min() < 3:
        j = int(np.argmax(lens < 3))
        raise PolygonError(f"feature {owner[j]}: a ring of {lens[j]} vertices")
    ring_first = np.concatenate([[0], np.cumsum(lens)])
    if ring_first[-1] > 1 << 24:
        raise PolygonError(f"{ring_first[-1]} vertices: at most 2^24")
    pts = np.concatenate(rings) if rings else np.zeros((0, 2))
    try:
        verts = quantise(pts)                                 # one pass over the image's vertices
    except PolygonError as e:
        bad = ~np.isfinite(pts).all(axis=1) | (np.abs(pts).max(axis=1) > MAX_COORD)
        j = int(np.searchsorted(ring_first, int(np.argmax(bad)), side="right")) - 1
        raise PolygonError(f"feature {owner[j]}: {e}") from None
    return {"verts": verts, "ring_first": ring_first.astype(np.int32), "poly_first_ring": np.asarray(poly_first, dtype=np.int32),
            "poly_label": np.asarray(labels, dtype=np.int32)}


def _load_geojson(path):
    try:
        feats = read_geojson(path)
    except (OSError, ValueError, KeyError, TypeError, AttributeError) as e:
        if isinstance(e, PolygonError):
            raise
        raise PolygonError(f"{path}: {e}") from None
    return pack(feats), len(feats)


def _load_features(feats, name):
    try:
        return pack(feats), len(feats)
    except PolygonError as e:
        raise PolygonError(f"{name}: {e}") from None


def find_polygons(path, images):
    """The annotations of the image files `images` under `path` -> {str(image path): load}, load() -> (packed record, number
    of features).  A directory holds NAME.geojson per image; a file is COCO, its images matched by the stem of file_name, and its
    width / height must be the image's (read from the header alone).  Checked HERE, before the caller starts: every annotation
    is there, and the COCO file is read and its sizes fit.  Reading and packing a GeoJSON file is left to load(), which a caller
    may run ahead on a thread; whatever a reader or pack refuses raises PolygonError there."""
    import functools
    from pathlib import Path
    src, found = Path(path), {}
    try:
        coco = None if src.is_dir() else read_coco(src)
    except (OSError, ValueError, KeyError, TypeError, AttributeError) as e:
        if isinstance(e, PolygonError):
            raise
        raise PolygonError(f"{src}: {e}") from None
    for img in map(Path, images):
        if coco is None:
            f = src / (img.stem + ".geojson")
            if not f.exists():
                raise PolygonError(f"no polygon file for {img.name} ({f})")
            found[str(img)] = functools.partial(_load_geojson, f)
        else:
            if img.stem not in coco:
                raise PolygonError(f"{src} lists no image with the stem {img.stem}")
            feats, (h, w) = coco[img.stem]
            from PIL import Image
            with Image.open(img) as a:
                if a.size != (w, h):
                    raise PolygonError(f"{src} gives {img.stem} as {w} x {h}, the image is {a.size[0]} x {a.size[1]}")
            found[str(img)] = functools.partial(_load_features, feats, f"{src}: {img.stem}")
    return found


def check_side(h, w):
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and h * w < 1 << 30):
        raise PolygonError(f"image {h} x {w}: sides 1..16384, h * w < 2^30")


# ---- the fill --------------------------------------------------------------------------------------------------------------------

def _edges(packed, p):
    """The edges of polygon p over all its rings, ordered so that y0 < y1, horizontal ones dropped: int64 x0, y0, x1, y1."""
    rf, pf = packed["ring_first"].astype(np.int64), packed["poly_first_ring"]
    first, end = rf[pf[p]:pf[p + 1]], rf[pf[p] + 1:pf[p + 1] + 1]
    if not len(first):
        z = np.zeros(0, np.int64)
        return z, z, z, z
    a, b = int(first[0]), int(end[-1])
    nxt = np.arange(a + 1, b + 1)
    nxt[end - 1 - a] = first                                  # the last vertex of a ring: back to its first
    v, u = packed["verts"][a:b].astype(np.int64), packed["verts"][nxt].astype(np.int64)
    x0, y0, x1, y1 = v[:, 0], v[:, 1], u[:, 0], u[:, 1]
    swap = y0 > y1
    x0, x1 = np.where(swap, x1, x0), np.where(swap, x0, x1)
    y0, y1 = np.where(swap, y1, y0), np.where(swap, y0, y1)
    keep = y0 < y1
    return x0[keep], y0[keep], x1[keep], y1[keep]


def polygon_box(x0, y0, x1, y1, h, w):
    """Rows r0..r1 (exclusive) whose centre line an edge can cross, and columns c0..c1 (exclusive) a toggle can start at, both
    clipped to the image: the box the device computes per polygon."""
    if not len(y0):
        return 0, 0, 0, 0
    ymin, ymax = int(y0.min()), int(y1.max())
    xmin, xmax = int(min(x0.min(), x1.min())), int(max(x0.max(), x1.max()))
    r0, r1 = (ymin - HALF + SUB - 1) >> 8, (ymax - HALF + SUB - 1) >> 8
    c0, c1 = ((xmin - HALF) >> 8) + 1, ((xmax - HALF) >> 8) + 1
    clip = lambda v, top: min(max(v, 0), top)
    return clip(r0, h), clip(r1, h), clip(c0, w), clip(c1, w)


def fill_polygon(x0, y0, x1, y1, box):
    """The inside mask of one polygon over its box, bool [r1 - r0, c1 - c0]: toggle columns by the formula for every (edge, row)
    crossing, then the prefix XOR along the row."""
    r0, r1, c0, c1 = box
    Y = SUB * np.arange(r0, r1, dtype=np.int64) + HALF
    cross = (y0[:, None] <= Y[None, :]) & (Y[None, :] < y1[:, None])
    e, r = np.nonzero(cross)
    dy = y1[e] - y0[e]
    k = ((Y[r] - y0[e]) * (x1[e] - x0[e]) + (x0[e] - HALF) * dy) // (SUB * dy) + 1
    k = np.clip(k, c0, c1) - c0                               # k = c1 toggles nothing inside the box
    span = c1 - c0
    t = (np.bincount(r * (span + 1) + k, minlength=(r1 - r0) * (span + 1)) & 1).astype(np.uint8).reshape(r1 - r0, span + 1)
    return np.bitwise_xor.accumulate(t, axis=1)[:, :span].astype(bool)


def census(labels):
    """-> (the positive values of the label map in ascending order, their pixel counts), both int64."""
    v, n = np.unique(np.asarray(labels), return_counts=True)
    keep = v > 0
    return v[keep].astype(np.int64), n[keep].astype(np.int64)


def rasterize_numpy(packed, h, w, compact=False):
    """-> {"labels": int32 [h, w], "kept": int64 [K], "area": int64 [K]}: the largest label among the polygons that contain the
    pixel's centre, 0 where none does; kept are the labels that own a pixel, ascending, area their pixel counts.  compact: the
    labels of the map are renumbered 1..K in that order (kept still holds the given ones)."""
    h, w = int(h), int(w)
    check_side(h, w)
    out = np.zeros((h, w), np.int32)
    lab = packed["poly_label"]
    for p in range(len(lab)):
        x0, y0, x1, y1 = _edges(packed, p)
        box = polygon_box(x0, y0, x1, y1, h, w)
        r0, r1, c0, c1 = box
        if r1 <= r0 or c1 <= c0:
            continue
        inside = fill_polygon(x0, y0, x1, y1, box)
        view = out[r0:r1, c0:c1]
        np.maximum(view, np.where(inside, lab[p], 0).astype(np.int32), out=view)
    kept, area = census(out)
    if compact and len(kept):
        out = np.where(out > 0, np.searchsorted(kept, out) + 1, 0).astype(np.int32)
    return {"labels": out, "kept": kept, "area": area}
