"""Droplet outlines as polygons: crack-following contours of a label map.

Pixel (r, c) is the square [c, c + 1] x [r, r + 1]; lattice corners are (x, y), x in 0..w, y in 0..h, y down.  A *crack* of
label k is a unit edge between a pixel of k and a pixel that is not k (or the outside of the image), directed so that the
k-pixel lies on its right hand on the screen; its id is (y_tail * (w + 1) + x_tail) * 4 + d with d = 0 E, 1 S, 2 W, 3 N.
The successor of a crack is found at its head, facing d: if the pixel ahead-right is not k turn right, else if the pixel
ahead-left is not k go straight, else turn left.  The cracks of a label fall into disjoint cycles, its *contours*; a contour
starts at its crack of smallest id, its vertices are the heads of the cracks whose successor has another direction, listed
from the start's tail, and its signed area S2 = sum (x_tail * y_head - x_head * y_tail) is positive for an outer contour
(clockwise on the screen) and negative for a hole.

``outlines_numpy`` is the host path of what ``unetdc_label_outlines`` computes on the device: a sequential crack follower.
``outline_columns`` is the ONE place where the integers become columns of the droplet table, for the device path, the CPU
path and the tests alike.  ``rings`` groups contours into polygons with holes; ``geojson`` and ``coco_annotation`` write them.
"""
import numpy as np

# the rows of unetdc_label_outlines, in its order (include/unetdc_hip.h)
QUANTITIES = ("E", "no", "nh", "nv", "F2", "S2")
# the columns of the contour table of unetdc_label_outlines, in its order
CONTOUR_FIELDS = ("label", "first", "nv", "length", "S2")
COLUMN_NAMES = ("perimeter_crack", "n_holes", "euler_number", "area_filled", "hole_area", "outline_vertices")
MICRON_COLUMN_NAMES = ("perimeter_crack_micron", "area_filled_sqmicron")
SUMMARY_NAMES = ("n_with_holes", "hole_area_total")

_DX, _DY = (1, 0, -1, 0), (0, 1, 0, -1)
# the pixels ahead-right and ahead-left of a head corner when facing d, as (row, column) offsets into the map padded by one
# pixel: the corner (x, y) has NW = P[y][x], NE = P[y][x + 1], SW = P[y + 1][x], SE = P[y + 1][x + 1]
_AR = ((1, 1), (1, 0), (0, 0), (0, 1))                     # E: SE, S: SW, W: NW, N: NE
_AL = ((0, 1), (1, 1), (1, 0), (0, 0))                     # E: NE, S: SE, W: SW, N: NW


def empty_record(n):
    return {"rows": {q: np.zeros(n, np.int64) for q in QUANTITIES},
            "contours": {f: np.zeros(0, np.int64) for f in CONTOUR_FIELDS},
            "x": np.zeros(0, np.int32), "y": np.zeros(0, np.int32)}


def outlines_numpy(labels, n=None):
    """labels: int [h, w], 0 = background, droplets 1..n (default labels.max()); labels outside that are skipped (for a
    droplet they are "not k" like the background).  -> the record
        rows      {E, no, nh, nv, F2, S2: int64 [n]}; a label without pixels keeps 0
        contours  {label, first, nv, length, S2: int64 [contours]} in ascending order of the start crack's id
        x, y      int32 [vertices]: contour i owns x[first[i] : first[i] + nv[i]], from its start's tail in walking order."""
    lab = np.asarray(labels)
    h, w = lab.shape
    n = int(lab.max(initial=0)) if n is None else int(n)
    rec = empty_record(n)
    pad = np.zeros((h + 2, w + 2), np.int64)
    pad[1:-1, 1:-1] = np.where((lab >= 1) & (lab <= n), lab, 0)
    nw, ne, sw, se = pad[:-1, :-1], pad[:-1, 1:], pad[1:, :-1], pad[1:, 1:]          # around every corner, [h + 1, w + 1]
    # the crack leaving a corner in direction d has its own pixel on the right (E: SE, S: SW, W: NW, N: NE) and another label
    # on the left (E: NE, S: SE, W: SW, N: NW); stacked last so that a flat index is the crack's id
    own, left = np.stack((se, sw, nw, ne), axis=-1), np.stack((ne, se, sw, nw), axis=-1)
    ids = np.flatnonzero((own > 0) & (own != left))
    if not len(ids):
        return rec
    P = pad.tolist()
    seen = np.zeros((h + 1) * (w + 1) * 4, bool)
    rows = {q: [0] * n for q in QUANTITIES}
    cont = {f: [] for f in CONTOUR_FIELDS}
    vx, vy = [], []
    for start in ids.tolist():
        if seen[start]:
            continue
        d, corner = start & 3, start >> 2
        x, y = corner % (w + 1), corner // (w + 1)
        k = P[y + _AR[d][0]][x + _AR[d][1]]                 # the pixel whose side this crack is: ahead-right of its tail
        length, s2, turns = 0, 0, []
        while True:                                          # the sequential follower: one crack per step
            seen[(y * (w + 1) + x) * 4 + d] = True
            hx, hy = x + _DX[d], y + _DY[d]
            length += 1
            s2 += x * hy - hx * y
            if P[hy + _AR[d][0]][hx + _AR[d][1]] != k:
                nd = (d + 1) & 3
            elif P[hy + _AL[d][0]][hx + _AL[d][1]] != k:
                nd = d
            else:
                nd = (d + 3) & 3
            if nd != d:
                turns.append((hx, hy))
            x, y, d = hx, hy, nd
            if (y * (w + 1) + x) * 4 + d == start:
                break
        turns = turns[-1:] + turns[:-1]                      # the last turn is the start's tail
        cont["label"].append(k), cont["first"].append(len(vx)), cont["nv"].append(len(turns))
        cont["length"].append(length), cont["S2"].append(s2)
        vx.extend(p[0] for p in turns), vy.extend(p[1] for p in turns)
        rows["E"][k - 1] += length
        rows["no" if s2 > 0 else "nh"][k - 1] += 1
        rows["nv"][k - 1] += len(turns)
        rows["F2"][k - 1] += s2 if s2 > 0 else 0
        rows["S2"][k - 1] += s2
    return {"rows": {q: np.array(rows[q], np.int64).reshape(n) for q in QUANTITIES},
            "contours": {f: np.array(cont[f], np.int64) for f in CONTOUR_FIELDS},
            "x": np.array(vx, np.int32), "y": np.array(vy, np.int32)}


def outline_columns(rec, area, px_per_um=None):
    """rec: the record of outlines_numpy (or of the device path) for droplets that each have at least one pixel; area: their
    pixel counts, which the signed areas must add up to (S2 = 2 area: a record of another label map is refused).  -> dict of
    the table's extra columns, in their order in the CSV: counts as int64, areas as float64.  A ratio is one correctly rounded
    division of Python integers.  perimeter_crack is a city-block length (a disc of radius r reads about 8 r, not 2 pi r)."""
    A = [int(v) for v in area]
    E, no, nh, nv, F2, S2 = ([int(v) for v in rec["rows"][q]] for q in QUANTITIES)
    if len(S2) != len(A) or any(s != 2 * a for s, a in zip(S2, A)):
        raise ValueError("outline_columns: the contours do not enclose the droplets' areas (another label map?)")
    cols = {"perimeter_crack": np.asarray(E, dtype=np.int64), "n_holes": np.asarray(nh, dtype=np.int64),
            "euler_number": np.asarray([o - q for o, q in zip(no, nh)], dtype=np.int64),
            "area_filled": np.array([f / 2 for f in F2], dtype=np.float64),
            "hole_area": np.array([(f - s) / 2 for f, s in zip(F2, S2)], dtype=np.float64),
            "outline_vertices": np.asarray(nv, dtype=np.int64)}
    if px_per_um is not None:
        cols["perimeter_crack_micron"] = cols["perimeter_crack"] / px_per_um
        cols["area_filled_sqmicron"] = cols["area_filled"] / (px_per_um * px_per_um)
    assert tuple(cols)[:len(COLUMN_NAMES)] == COLUMN_NAMES and all(len(v) == len(A) for v in cols.values())
    return cols


def outline_summary(cols):
    """The two per-image summary values of SUMMARY_NAMES from outline_columns' result."""
    return {"n_with_holes": int(np.count_nonzero(cols["n_holes"])), "hole_area_total": float(np.sum(cols["hole_area"]))}


def ring(rec, i, closed=False):
    """The vertices of contour i as a list of [x, y] Python integers; closed: the first vertex once more at the end."""
    a, m = int(rec["contours"]["first"][i]), int(rec["contours"]["nv"][i])
    pts = np.stack((rec["x"][a:a + m], rec["y"][a:a + m]), axis=1).tolist()
    return pts + pts[:1] if closed else pts


def inside(pts, px, py):
    """Even-odd crossing test of the point (px, py) against the polygon pts, for a point on no edge (a pixel centre against
    lattice vertices): the ray towards +x crosses an odd number of the polygon's vertical edges."""
    hit = False
    for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
        if x0 == x1 and x0 > px and min(y0, y1) < py < max(y0, y1):        # every edge is axis-parallel
            hit = not hit
    return hit


def _start_pixel(pts):
    """The centre of the pixel on the right hand of a contour's first crack (a pixel of its label), from its first two vertices."""
    (x0, y0), (x1, y1) = pts[0], pts[1]
    d = 0 if x1 > x0 else 2 if x1 < x0 else 1 if y1 > y0 else 3
    r, c = (y0, x0) if d == 0 else (y0, x0 - 1) if d == 1 else (y0 - 1, x0 - 1) if d == 2 else (y0 - 1, x0)
    return c + 0.5, r + 0.5


def rings(rec):
    """{label: [(outer contour index, [hole contour indices]), ...]} in the contours' order.  A hole belongs to the outer
    contour of its label that contains it: the even-odd test is made at the centre of the label's pixel beside the hole's start
    crack (a vertex could lie on a contour of a neighbouring piece), and among nested outer contours the innermost (smallest
    S2) is taken.  A label with one outer contour, as every droplet of the quantification flow, is not tested at all."""
    c = rec["contours"]
    out, holes = {}, {}
    for i, (k, s2) in enumerate(zip(c["label"].tolist(), c["S2"].tolist())):         # plain integers from here on
        if s2 > 0:
            out.setdefault(k, []).append((i, []))
        else:
            holes.setdefault(k, []).append(i)
    for k, hs in holes.items():
        outers = out[k]
        polys = {i: ring(rec, i) for i, _ in outers} if len(outers) > 1 else None
        for hi in hs:
            if polys is None:
                outers[0][1].append(hi)
                continue
            px, py = _start_pixel(ring(rec, hi))
            best = min((j for j in range(len(outers)) if inside(polys[outers[j][0]], px, py)),
                       key=lambda j: int(c["S2"][outers[j][0]]))
            outers[best][1].append(hi)
    return dict(sorted(out.items()))


def _closed_rings(rec):
    """Every contour as a closed list of [x, y]: one gather and one tolist for the image, then list slices."""
    first, nv = rec["contours"]["first"], rec["contours"]["nv"]
    m = nv + 1
    start = np.cumsum(m) - m
    idx = np.arange(int(m.sum())) - np.repeat(start - first, m)       # first .. first + nv of every contour
    idx[start + nv] = first                                           # where the last step is the first vertex again
    pts = np.stack((rec["x"], rec["y"]), axis=1)[idx].tolist()
    return [pts[a:b] for a, b in zip(start.tolist(), (start + m).tolist())]


def geojson(rec, name, px_per_um=None, groups=None):
    """A GeoJSON FeatureCollection (a dict for json.dump): one Feature per label with pixels, a Polygon or, for a label of
    several pieces, a MultiPolygon; rings are closed lists of [x, y] in pixel coordinates (y down, as on the screen), the outer
    ring first, then its holes.  Properties: label, area (pixels) and with px_per_um area_sqmicron.  How QuPath, napari or CVAT
    orient or clip such rings on import is not pinned by any test here.  groups: rings(rec), where the caller has it."""
    feats = []
    closed = _closed_rings(rec)
    areas = (rec["rows"]["S2"] // 2).tolist()
    for k, polys in (rings(rec) if groups is None else groups).items():
        coords = [[closed[o]] + [closed[i] for i in hs] for o, hs in polys]
        props = {"label": k, "area": areas[k - 1]}
        if px_per_um is not None:
            props["area_sqmicron"] = areas[k - 1] / (px_per_um * px_per_um)
        geom = {"type": "Polygon", "coordinates": coords[0]} if len(coords) == 1 else {"type": "MultiPolygon", "coordinates": coords}
        feats.append({"type": "Feature", "id": k, "properties": props, "geometry": geom})
    return {"type": "FeatureCollection", "name": str(name), "features": feats}


def coco_annotation(rec, image_id=1, category_id=1, first_id=1, groups=None):
    """COCO annotations (a list of dicts), one per label with pixels: segmentation = the outer rings only, each a flat
    [x0, y0, x1, y1, ...] list (a COCO polygon cannot express a hole), area = the pixel count, bbox = [x, y, width, height]
    of the vertices, and the number of holes left out under the extra key "holes".  groups: rings(rec), where the caller has it."""
    anns = []
    c = rec["contours"]
    if not len(c["label"]):
        return anns
    flat = np.stack((rec["x"], rec["y"]), axis=1).ravel().tolist()
    first, ends = c["first"].tolist(), (c["first"] + c["nv"]).tolist()
    x0, x1 = np.minimum.reduceat(rec["x"], c["first"]).tolist(), np.maximum.reduceat(rec["x"], c["first"]).tolist()
    y0, y1 = np.minimum.reduceat(rec["y"], c["first"]).tolist(), np.maximum.reduceat(rec["y"], c["first"]).tolist()
    area, holes = (rec["rows"]["S2"] // 2).tolist(), rec["rows"]["nh"].tolist()
    for k, polys in (rings(rec) if groups is None else groups).items():
        outer = [o for o, _ in polys]
        seg = [flat[2 * first[o]:2 * ends[o]] for o in outer]
        bx, by = min(x0[o] for o in outer), min(y0[o] for o in outer)
        anns.append({"id": first_id + len(anns), "image_id": image_id, "category_id": category_id, "segmentation": seg,
                     "area": area[k - 1], "bbox": [bx, by, max(x1[o] for o in outer) - bx, max(y1[o] for o in outer) - by],
                     "iscrowd": 0, "holes": holes[k - 1], "label": k})
    return anns
