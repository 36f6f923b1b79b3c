"""Object-level agreement of two label maps: predicted droplets against annotated ones.

``overlap_table_numpy`` is the host path of what ``unetdc_label_overlap`` computes on the device: the sparse contingency
table of two int32 label maps, in ascending (a, b) order.  ``match_columns`` is the ONE place where that table and the two
area lists become matches, merged / split / missed / spurious counts and the float64 columns, for the device path, the CPU
path and the tests alike; ``summary_row`` and ``pooled_row`` build the rows of ``match_per_image.csv``.  Every decision is
an integer comparison; no float decides anything.
"""
import numpy as np

THRESHOLDS = tuple(range(10, 20))            # k: a match at IoU threshold k / 20 is 20 n > k U, strict
TP_NAMES = tuple(f"tp_{5 * k}" for k in THRESHOLDS)
AP_NAMES = tuple(f"ap_{5 * k}" for k in THRESHOLDS)
COUNT_NAMES = ("n_pred", "n_gt", "n_merged", "n_split", "n_missed", "n_spurious") + TP_NAMES
PIXEL_NAMES = ("inter_px", "pred_px", "gt_px")
INTEGER_NAMES = COUNT_NAMES + PIXEL_NAMES


def overlap_table_numpy(A, B, ka, kb):
    """A, B: int label maps of one shape (0 = background, objects 1..ka and 1..kb) -> int64 arrays (a, b, n): the pairs that
    share a pixel and the number of shared pixels, in ascending order of (a, b).  Pixels whose label is below 1 or above
    ka (kb) on either side contribute nothing."""
    a = np.asarray(A).ravel().astype(np.int64)
    b = np.asarray(B).ravel().astype(np.int64)
    if a.shape != b.shape:
        raise ValueError("the two label maps differ in size")
    both = (a >= 1) & (a <= int(ka)) & (b >= 1) & (b <= int(kb))
    keys, n = np.unique((a[both] << 32) | b[both], return_counts=True)
    return keys >> 32, keys & 0xFFFFFFFF, n.astype(np.int64)


def _count_per(index, where, size):
    return np.bincount(index[where] - 1, minlength=size).astype(np.int64)[:size]


def match_columns(areaA, areaB, a, b, n):
    """areaA [Ka], areaB [Kb]: the areas of the objects 1..Ka of the first map (the prediction) and 1..Kb of the second (the
    annotation); a, b, n: their overlap table.  -> dict with
      "pred":  gt_label (partner at IoU > 1/2, else 0), gt_iou (n / U, one division; 0.0 without a partner), gt_covered
               (annotated objects mostly inside this prediction), one entry per predicted object;
      "gt":    pred_label, pred_iou, pred_covered, the same mirrored, one entry per annotated object;
      "image": the integers of INTEGER_NAMES (summary_row derives the ratios from them)."""
    areaA, areaB = np.asarray(areaA, dtype=np.int64), np.asarray(areaB, dtype=np.int64)
    a, b, n = (np.asarray(v, dtype=np.int64) for v in (a, b, n))
    ka, kb = len(areaA), len(areaB)
    U = areaA[a - 1] + areaB[b - 1] - n
    match = [20 * n > k * U for k in THRESHOLDS]
    m = match[0]                                           # IoU > 1/2: at most one partner on either side
    gt_label, pred_label = np.zeros(ka, np.int64), np.zeros(kb, np.int64)
    gt_iou, pred_iou = np.zeros(ka, np.float64), np.zeros(kb, np.float64)
    iou = n[m] / U[m]
    gt_label[a[m] - 1], gt_iou[a[m] - 1] = b[m], iou
    pred_label[b[m] - 1], pred_iou[b[m] - 1] = a[m], iou
    merges = _count_per(a, 2 * n > areaB[b - 1], ka)
    splits = _count_per(b, 2 * n > areaA[a - 1], kb)
    image = {"n_pred": ka, "n_gt": kb, "n_merged": int((merges >= 2).sum()), "n_split": int((splits >= 2).sum()),
             "n_missed": kb - len(np.unique(b)), "n_spurious": ka - len(np.unique(a))}
    image.update((name, int(mk.sum())) for name, mk in zip(TP_NAMES, match))
    image.update(inter_px=int(n.sum()), pred_px=int(areaA.sum()), gt_px=int(areaB.sum()))
    return {"pred": {"gt_label": gt_label, "gt_iou": gt_iou, "gt_covered": merges},
            "gt": {"pred_label": pred_label, "pred_iou": pred_iou, "pred_covered": splits}, "image": image}


def _ratio(num, den, nothing):
    """A ratio with a zero denominator is 0.0 -- but where neither map holds an object, every ratio is 1.0."""
    return 1.0 if nothing else (num / den if den else 0.0)


def summary_row(filename, image):
    """The row of match_per_image.csv from the integers of match_columns(...)["image"] (or their sums over images)."""
    ka, kb = int(image["n_pred"]), int(image["n_gt"])
    nothing = ka == 0 and kb == 0
    row = {"filename": filename}
    row.update((q, int(image[q])) for q in COUNT_NAMES)
    tp = row["tp_50"]
    row["precision_50"] = _ratio(tp, ka, nothing)
    row["recall_50"] = _ratio(tp, kb, nothing)
    row["f1_50"] = _ratio(2 * tp, ka + kb, nothing)
    total = 0.0
    for tname, aname in zip(TP_NAMES, AP_NAMES):           # summed in the order k = 10..19
        row[aname] = _ratio(row[tname], ka + kb - row[tname], nothing)
        total += row[aname]
    row["mean_ap"] = total / 10
    row.update((q, int(image[q])) for q in PIXEL_NAMES)
    inter, px = row["inter_px"], row["pred_px"] + row["gt_px"]
    row["pixel_dice"] = _ratio(2 * inter, px, nothing)
    row["pixel_iou"] = _ratio(inter, px - inter, nothing)
    return row


def pooled_row(images, filename="ALL"):
    """The row of the integer columns summed over the images; its ratios come from those sums."""
    return summary_row(filename, {q: sum(int(im[q]) for im in images) for q in INTEGER_NAMES})


def label_sums(labels, k=None):
    """int label map -> (area, sum of rows, sum of columns) as int64 [k] for the labels 1..k (k = labels.max() by default)."""
    lab = np.asarray(labels)
    h, w = lab.shape
    k = int(lab.max(initial=0)) if k is None else int(k)
    flat = lab.ravel()
    idx = np.flatnonzero((flat >= 1) & (flat <= k))
    v = flat[idx].astype(np.int64)
    # float64 weights are exact here: every partial sum is an integer below 2^53
    area = np.bincount(v, minlength=k + 1)[1:].astype(np.int64)
    sy = np.bincount(v, weights=(idx // w).astype(np.float64), minlength=k + 1)[1:].astype(np.int64)
    sx = np.bincount(v, weights=(idx % w).astype(np.float64), minlength=k + 1)[1:].astype(np.int64)
    return area, sy, sx


def gt_labels_numpy(mask, min_area=1):
    """Binary annotation -> its int32 label map: 4-connected components of at least min_area pixels, numbered in raster
    order of their first pixel (what unetdc_ccl_labels writes).  The annotation is never split."""
    from scipy import ndimage
    lbl, k = ndimage.label(np.asarray(mask) > 0)
    if k:
        keep = np.bincount(lbl.ravel(), minlength=k + 1) >= max(int(min_area), 1)
        keep[0] = False
        lbl = ndimage.label(keep[lbl])[0]
    return lbl.astype(np.int32)


def gt_table(filename, area, sy, sx, gt_cols):
    """The rows of gt_droplets.csv for one image, as a dict of columns."""
    k = len(area)
    d = np.maximum(area, 1)
    out = {"filename": [filename] * k, "label": np.arange(1, k + 1), "area": np.asarray(area, dtype=np.int64),
           "centroid-0": np.asarray(sy, dtype=np.float64) / d, "centroid-1": np.asarray(sx, dtype=np.float64) / d}
    out.update(gt_cols)
    return out
