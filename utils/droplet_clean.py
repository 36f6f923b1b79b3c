"""Host path of the mask-cleaning stage: hysteresis threshold and hole filling of a {0,1} mask on
numpy with scipy.ndimage.label (default cross-shaped structure = 4-connectivity).  The device path is csrc/clean.hip
(unetdc_mask_clean), the plain-loop restatement tests/clean_ref.py; the three agree bit for bit.  The CPU path of
quantify_droplets_batch.py calls clean_mask."""
import numpy as np
from scipy import ndimage

COUNT_NAMES = ("hysteresis_added_px", "holes_filled", "hole_px_filled", "holes_left_open")


def clean_mask(strong, weak=None, max_hole_area=0):
    """strong, weak (or None): [h, w] arrays, nonzero = 1.  max_hole_area: 0 = do not fill, negative = fill holes of any size,
    N > 0 = fill holes of at most N pixels.  -> (uint8 {0,1} mask, int64 [4] counts: pixels of the hysteresis mask not in
    strong, holes filled, pixels filled, holes left open because of their size)."""
    s = np.asarray(strong) != 0
    added = filled = pixels = left = 0
    if weak is None:
        m = s
    else:
        lab, n = ndimage.label(np.asarray(weak) != 0)
        seeded = np.zeros(n + 1, bool)
        seeded[lab[s]] = True                           # lab is 0 where strong lies outside weak
        seeded[0] = False
        m = seeded[lab]
        added = int(np.count_nonzero(m & ~s))
    if max_hole_area != 0:
        lab, n = ndimage.label(~m)
        border = np.zeros(n + 1, bool)
        for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
            border[edge] = True
        area = np.bincount(lab.ravel(), minlength=n + 1)
        hole = ~border
        hole[0] = False
        fill = hole if max_hole_area < 0 else hole & (area <= max_hole_area)
        filled, pixels, left = int(fill.sum()), int(area[fill].sum()), int((hole & ~fill).sum())
        m = m | fill[lab]
    return m.astype(np.uint8), np.array([added, filled, pixels, left], np.int64)
