"""Brute-force oracle of the droplets-per-cell stage (csrc/cells.hip, utils/droplet_cells.py), written from the definitions in
include/unetdc_hip.h alone: it shares no code with utils/droplet_cells.py.

nearest_brute: for every pixel the minimum over ALL seed pixels of d2 * 2^20 + label (labels below 2^20), a chunk of pixels at
a time.  cell_table_brute: plain loops over the pixels."""
import numpy as np

EDT_INF = 2 ** 31 - 1
LABEL_BITS = 20


def nearest_brute(label, max_label, radius=0, chunk=4096, rows=None):
    """-> (out_label int32 [h, w], out_d2 int32 [h, w]); rows: only these rows of the image are computed (the planes are then
    [len(rows), w]): what a large image can afford."""
    label = np.asarray(label).astype(np.int64)
    h, w = label.shape
    assert max_label < (1 << LABEL_BITS)
    sy, sx = np.nonzero((label >= 1) & (label <= max_label))
    if len(sy) == 0:
        h = h if rows is None else len(rows)
        return np.zeros((h, w), np.int32), np.full((h, w), EDT_INF, np.int32)
    sl = label[sy, sx]
    if rows is None:
        py, px = np.divmod(np.arange(h * w, dtype=np.int64), w)
    else:
        py, px, h = np.repeat(np.asarray(rows, np.int64), w), np.tile(np.arange(w, dtype=np.int64), len(rows)), len(rows)
    key = np.empty(h * w, np.int64)
    chunk = max(1, min(chunk, (1 << 24) // len(sy)))                 # at most 2^24 (pixel, seed) pairs at a time
    for s in range(0, h * w, chunk):
        dy = py[s:s + chunk, None] - sy[None, :]
        dx = px[s:s + chunk, None] - sx[None, :]
        key[s:s + chunk] = (((dy * dy + dx * dx) << LABEL_BITS) + sl[None, :]).min(axis=1)
    d2 = (key >> LABEL_BITS).reshape(h, w)
    lab = (key & ((1 << LABEL_BITS) - 1)).reshape(h, w)
    if radius > 0:
        lab = np.where(d2 > radius * radius, 0, lab)
    return lab.astype(np.int32), d2.astype(np.int32)


def cell_table_brute(droplet_label, max_droplet, cell_label, max_cell, d2=None):
    """-> (out_droplet int32 [6, max_droplet], out_cell int64 [8, max_cell], the number of (droplet, cell) pairs)."""
    a_map, b_map = np.asarray(droplet_label), np.asarray(cell_label)
    h, w = a_map.shape
    od = [[0, 0, 0, 0, 0, EDT_INF] for _ in range(max_droplet)]
    oc = [[0] * 8 for _ in range(max_cell)]
    pairs = {}
    for y in range(h):
        for x in range(w):
            a, b = int(a_map[y, x]), int(b_map[y, x])
            a = a if 1 <= a <= max_droplet else 0
            b = b if 1 <= b <= max_cell else 0
            d = None if d2 is None else int(d2[y, x])
            if a:
                od[a - 1][4] += 1
                od[a - 1][3] += b == 0
                if d is not None:
                    od[a - 1][5] = min(od[a - 1][5], d)
            if b:
                oc[b - 1][0] += 1
                oc[b - 1][1] += y in (0, h - 1) or x in (0, w - 1)
                oc[b - 1][2] += a != 0
                oc[b - 1][7] += d == 0
            if a and b:
                pairs[(a, b)] = pairs.get((a, b), 0) + 1
    for a in range(1, max_droplet + 1):
        mine = sorted((-n, b) for (aa, b), n in pairs.items() if aa == a)       # most pixels first, then the smallest cell
        od[a - 1][2] = len(mine)
        if mine:
            od[a - 1][0], od[a - 1][1] = mine[0][1], -mine[0][0]
            c, area = oc[mine[0][1] - 1], od[a - 1][4]
            c[3] += 1
            c[4] += area
            c[5] += area * area
            c[6] = max(c[6], area)
    out_d = np.array(od, np.int32).reshape(max_droplet, 6).T.copy()
    out_c = np.array(oc, np.int64).reshape(max_cell, 8).T.copy()
    return out_d, out_c, len(pairs)


# ---- the cases both test files run -----------------------------------------------------------------------------------------------

def nearest_cases():
    """{name: (label int32 [h, w], max_label)}: the cases of the nearest-label transform that CPU and device share."""
    c = {}
    row = np.zeros((1, 7), np.int32)
    row[0, 0], row[0, 6] = 2, 1
    c["row_tie"] = (row, 2)
    col = np.zeros((5, 7), np.int32)
    col[0, 3], col[4, 3] = 5, 2
    c["column_tie"] = (col, 5)
    c["random_seeds"] = (random_seeds(37, 53, 40, 0), 40)
    c["no_seed"] = (np.zeros((6, 9), np.int32), 3)
    c["all_seeds"] = (np.arange(1, 6 * 9 + 1, dtype=np.int32).reshape(6, 9), 54)
    out = random_seeds(11, 17, 12, 1)
    out[2, 3], out[7, 9], out[10, 16] = 99, -4, 13                  # above max_label, below 1, just above: none is a seed
    c["out_of_range"] = (out, 12)
    blocks = np.zeros((12, 20), np.int32)
    blocks[3:8, 4:9], blocks[3:8, 9:13], blocks[8:10, 6:12] = 7, 3, 5
    c["touching_blocks"] = (blocks, 7)
    return c


def random_seeds(h, w, n, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros(h * w, np.int32)
    lab[rng.choice(h * w, n, replace=False)] = rng.permutation(n) + 1
    return lab.reshape(h, w)


def table_cases():
    """{name: (droplet int32 [h, w], max_droplet, cell int32 [h, w], max_cell)}: one image that holds every case of the cell
    table, and the degenerate limits."""
    h, w = 14, 18
    cell, drop = np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
    cell[0:6, 0:6] = 1                                   # on the image border
    cell[2:8, 8:11], cell[2:8, 11:14] = 4, 2             # two cells side by side
    cell[8:12, 8:14] = 3
    cell[10:13, 1:5] = 5                                 # a cell without droplets
    cell[0:2, 15:18] = 9                                 # above max_cell: background
    drop[1:3, 1:4] = 1                                   # wholly inside cell 1
    drop[3:5, 9:12] = 2                                  # four pixels on cell 4, one on cell 2 ...
    drop[3, 11] = 0                                      # ... once this one is gone
    drop[5:6, 8:14] = 3                                  # 3 / 3 between cells 4 and 2: goes to cell 2
    drop[12:14, 15:18] = 4                               # outside any cell
    drop[7:9, 10:13] = 5                                 # over cells 4, 2 and 3
    drop[0:2, 16:18] = 6                                 # on the out-of-range cell label: outside
    drop[6, 2:4] = 12                                    # above max_droplet: background
    c = {"mixed": (drop, 7, cell, 5)}
    c["no_droplets"] = (drop, 0, cell, 5)
    c["no_cells"] = (drop, 7, cell, 0)
    c["nothing"] = (drop, 0, cell, 0)
    return c
