"""Pixel scores of the thresholded mask against an annotation at every threshold of a grid.

The mask rule (strict ``>`` on the fp32 probability, then the resize of ``droplets.py``) is monotone in the threshold, so an
output pixel has one *level*: the number of grid thresholds at which it is set.  ``hist[g][level]`` (g = annotated) therefore
holds the confusion matrix at every threshold.  ``sweep_hist_numpy`` is the host path of what ``unetdc_thresh_sweep`` adds up
on the device; ``sweep_table`` is the ONE place where a histogram becomes precision / recall / Dice / IoU, the average
precision and the best thresholds, for the device path, the CPU path and the tests alike.  Only numpy is needed here.
"""
import numpy as np

MAX_K = 1024
COLUMNS = ("k", "threshold", "tp", "fp", "fn", "tn", "precision", "recall", "dice", "iou")


def grid(K):
    """The K thresholds t_k = (float)k / (float)K as float32: one correctly rounded division each."""
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"K = {K} outside 1..{MAX_K}")
    return np.arange(K, dtype=np.float32) / np.float32(K)


def level_hist(level, gt, K):
    """level: int array in 0..K; gt: array of the same shape (nonzero = annotated) -> int64 [2][K + 1]."""
    level, g = np.asarray(level).ravel().astype(np.int64), (np.asarray(gt).ravel() != 0).astype(np.int64)
    if level.shape != g.shape:
        raise ValueError("the annotation differs in size from the mask")
    return np.bincount(g * (K + 1) + level, minlength=2 * (K + 1)).astype(np.int64).reshape(2, K + 1)


def sweep_hist_numpy(probs2d, gt, out_hw, K, linear=True):
    """probs2d: fp32 [ph, pw]; gt: [oh, ow] (nonzero = annotated); -> int64 [2][K + 1].  A plain loop over the grid: the mask
    of every threshold, resized as the script's CPU path resizes it (linear: resize_mask_like_reference; else the nearest
    rule), summed into the level."""
    from unet_dc_segmentation_amd.droplets import resize_mask_like_reference, resize_nearest_cv2
    p = np.asarray(probs2d, dtype=np.float32)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if tuple(np.shape(gt)) != (oh, ow):
        raise ValueError(f"the annotation is {tuple(np.shape(gt))}, the output size {(oh, ow)}")
    level = np.zeros((oh, ow), np.int64)
    t = grid(K)
    step = max(1, min(64, (1 << 22) // (oh * ow)))        # several thresholds per resize call, as channels of one image
    with np.errstate(invalid="ignore"):
        for k in range(0, len(t), step):
            m = (p[:, :, None] > t[None, None, k:k + step]).astype(np.uint8)      # a NaN is never set
            r = resize_mask_like_reference(m, ow, oh) if linear else resize_nearest_cv2(m, ow, oh)
            level += (r != 0).sum(axis=2)
    return level_hist(level, gt, int(K))


def _ratio(num, den, nothing):
    """Element-wise num / den in float64; 0.0 where den is 0 -- but 1.0 wherever the data hold neither an annotated nor a
    predicted pixel (the convention of utils/droplet_match.py)."""
    out = np.zeros(len(num), np.float64)
    np.divide(num, den, out=out, where=den != 0)
    out[nothing] = 1.0
    return out


def sweep_table(hist):
    """hist: int [2][K + 1] -> dict: per k the arrays threshold (fp32 grid as float64), tp, fp, fn, tn (int64), precision,
    recall, dice, iou (float64); and the scalars K, average_precision, best_dice_k, best_iou_k (the smallest k of the
    maximum)."""
    h = np.asarray(hist, dtype=np.int64)
    if h.ndim != 2 or h.shape[0] != 2 or h.shape[1] < 2:
        raise ValueError("hist must be [2][K + 1]")
    K = h.shape[1] - 1
    above = h[:, ::-1].cumsum(axis=1)[:, ::-1]             # above[g][l] = sum over levels >= l
    tp, fp = above[1, 1:], above[0, 1:]                    # levels > k, k = 0..K-1
    fn, tn = above[1, 0] - tp, above[0, 0] - fp
    nothing = (tp + fp + fn) == 0
    f = np.float64
    precision = _ratio(tp.astype(f), (tp + fp).astype(f), nothing)
    recall = _ratio(tp.astype(f), (tp + fn).astype(f), nothing)
    dice = _ratio((2 * tp).astype(f), (2 * tp + fp + fn).astype(f), nothing)
    iou = _ratio(tp.astype(f), (tp + fp + fn).astype(f), nothing)
    ap = 0.0
    for k in range(K):                                     # summed in the order k = 0..K-1; recall_K = 0
        ap += (recall[k] - (recall[k + 1] if k + 1 < K else 0.0)) * precision[k]
    return {"K": K, "threshold": grid(K).astype(f), "tp": tp, "fp": fp, "fn": fn, "tn": tn, "precision": precision,
            "recall": recall, "dice": dice, "iou": iou, "average_precision": float(ap),
            "best_dice_k": int(np.argmax(dice)), "best_iou_k": int(np.argmax(iou))}


def table_rows(hist):
    """The rows of threshold_sweep.csv: one dict per k with the columns COLUMNS."""
    t = sweep_table(hist)
    rows = []
    for k in range(t["K"]):
        row = {"k": k}
        row.update((c, (int if c in ("tp", "fp", "fn", "tn") else float)(t[c][k])) for c in COLUMNS[1:])
        rows.append(row)
    return rows


def summary_line(hist):
    """One line for the console: the Dice-optimal threshold, its pooled Dice and the average precision."""
    t = sweep_table(hist)
    k = t["best_dice_k"]
    return (f"Threshold sweep (K = {t['K']}): best pooled Dice {t['dice'][k]:.4f} at threshold {t['threshold'][k]:.6g} "
            f"(k = {k}); average precision {t['average_precision']:.4f}")
