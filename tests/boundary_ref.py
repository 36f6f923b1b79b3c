"""Plain-loop restatement of DESIGN.md section 21 (surface distances between two label maps), written from the definition alone:
lists of lists in, Python integers out, no numpy, no distance transform.  The nearest boundary pixel is searched row by row
outward from the query's row, and the search stops once the row offset alone is no closer than the best so far; within a row
every boundary pixel is tried.  For small sides only."""
import math

INF = 2147483647


def label_at(L, k, y, x):
    v = L[y][x]
    return v if 1 <= v <= k else 0


def boundary_pixels(L, k):
    """[(y, x, label)] in raster order: a label in 1..k whose 4-neighbour lies outside the image or carries another value."""
    h, w = len(L), len(L[0])
    out = []
    for y in range(h):
        for x in range(w):
            a = label_at(L, k, y, x)
            if a == 0:
                continue
            edge = False
            for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if ny < 0 or ny >= h or nx < 0 or nx >= w or label_at(L, k, ny, nx) != a:
                    edge = True
            if edge:
                out.append((y, x, a))
    return out


def nearest_d2(p, rows, h):
    """min over q of |p - q|^2, q from rows (row -> list of columns), INF without any q."""
    y, x = p
    best = INF
    for dy in range(h):
        if dy * dy >= best:
            break
        for yy in ((y,) if dy == 0 else (y - dy, y + dy)):
            for xx in rows.get(yy, ()):
                d = dy * dy + (x - xx) * (x - xx)
                if d < best:
                    best = d
    return best


def distances(A, ka, B, kb):
    """-> ([(label, d2)] for the boundary pixels of A against those of B, the same for B against A)."""
    h = len(A)
    pa, pb = boundary_pixels(A, ka), boundary_pixels(B, kb)
    out = []
    for mine, other in ((pa, pb), (pb, pa)):
        rows = {}
        for y, x, _ in other:
            rows.setdefault(y, []).append(x)
        out.append([(k, nearest_d2((y, x), rows, h)) for y, x, k in mine])
    return out


def record_ref(A, ka, B, kb, R, dist=None):
    """The record of section 21 as plain lists: hist [2][R^2 + 2], dmax [2], tables [3][ka] and [3][kb]."""
    dist = distances(A, ka, B, kb) if dist is None else dist
    far = R * R + 1
    hist, dmax, tables = [[0] * (far + 1) for _ in range(2)], [-1, -1], []
    for d, k_side in ((0, ka), (1, kb)):
        t = [[0] * k_side, [-1] * k_side, [0] * k_side]
        for k, d2 in dist[d]:
            hist[d][min(d2, far)] += 1
            dmax[d] = max(dmax[d], d2)
            t[0][k - 1] += 1
            t[1][k - 1] = max(t[1][k - 1], d2)
            t[2][k - 1] += d2
        tables.append(t)
    return {"hist": hist, "dmax": dmax, "a": tables[0], "b": tables[1]}


def columns_ref(hist, dmax, R, tols=(1, 2, 3)):
    """The derived numbers of section 21 from the record."""
    n = [sum(hist[0]), sum(hist[1])]
    empty = n[0] == 0 and n[1] == 0
    out = {"bd_px_pred": n[0], "bd_px_gt": n[1], "n_far_pred": hist[0][R * R + 1], "n_far_gt": hist[1][R * R + 1]}
    top = max(dmax)
    out["hd"] = 0.0 if empty else (math.inf if top == INF else math.sqrt(top))
    per_dir = []
    for d in (0, 1):
        if n[d] == 0:
            per_dir.append(0.0)
            continue
        need = -((-95 * n[d]) // 100)                      # ceil(95 n / 100)
        cum = 0
        for l in range(R * R + 2):
            cum += hist[d][l]
            if cum >= need:
                per_dir.append(math.sqrt(min(l, R * R)))
                break
    out["hd95"] = max(per_dir)
    out["assd"] = 0.0 if empty else math.fsum(hist[d][l] * math.sqrt(min(l, R * R)) for d in (0, 1) for l in range(R * R + 2)) / (n[0] + n[1])
    for t in tols:
        c = [sum(hist[d][l] for l in range(R * R + 2) if l <= t * t) for d in (0, 1)]
        pairs = (("bprec", c[0], n[0]), ("brec", c[1], n[1]), ("bf", 2 * c[0] * c[1], c[0] * n[1] + c[1] * n[0]),
                 ("nsd", c[0] + c[1], n[0] + n[1]))
        for name, num, den in pairs:
            out[f"{name}_{t}"] = 1.0 if empty else (num / den if den else 0.0)
    return out


def object_ref(table):
    """[(bd_px, bd_rms, bd_max)] per object; None for the two floats of an object without a boundary pixel."""
    out = []
    for cnt, mx, sm in zip(*table):
        if cnt == 0:
            out.append((0, None, None))
        elif mx == INF:
            out.append((cnt, math.inf, math.inf))
        else:
            out.append((cnt, math.sqrt(sm / cnt), math.sqrt(mx)))
    return out
