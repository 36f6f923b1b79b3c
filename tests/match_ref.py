"""Plain-loop restatement of DESIGN.md section 12 (overlap table of two label maps, IoU matching, merged / split / missed /
spurious counts, the per-image row), written from the text alone: Python lists, integers and one division per ratio.
Slow on purpose; the vectorised path (utils/droplet_match.py) and the device kernel (csrc/match.hip) are tested against it."""


def overlap_table_ref(A, B, ka, kb):
    """A, B: lists of rows of integers.  -> [(a, b, n)] in ascending order of (a, b)."""
    counts = {}
    for row_a, row_b in zip(A, B):
        for a, b in zip(row_a, row_b):
            if 1 <= a <= ka and 1 <= b <= kb:
                counts[(a, b)] = counts.get((a, b), 0) + 1
    return [(a, b, counts[(a, b)]) for a, b in sorted(counts)]


def match_ref(area_a, area_b, triples):
    """area_a[a - 1], area_b[b - 1]: the areas; triples: the overlap table.  -> (per-A rows [(gt_label, gt_iou, gt_covered)],
    per-B rows [(pred_label, pred_iou, pred_covered)], dict of the per-image integers)."""
    ka, kb = len(area_a), len(area_b)
    pred = [[0, 0.0, 0] for _ in range(ka)]
    gt = [[0, 0.0, 0] for _ in range(kb)]
    tp = {k: 0 for k in range(10, 20)}
    seen_a, seen_b = set(), set()
    inter = 0
    for a, b, n in triples:
        assert n > 0
        u = area_a[a - 1] + area_b[b - 1] - n
        for k in range(10, 20):
            if 20 * n > k * u:
                tp[k] += 1
        if 20 * n > 10 * u:
            assert pred[a - 1][0] == 0 and gt[b - 1][0] == 0          # above one half: at most one partner
            pred[a - 1][0], pred[a - 1][1] = b, n / u
            gt[b - 1][0], gt[b - 1][1] = a, n / u
        if 2 * n > area_b[b - 1]:
            pred[a - 1][2] += 1
        if 2 * n > area_a[a - 1]:
            gt[b - 1][2] += 1
        seen_a.add(a)
        seen_b.add(b)
        inter += n
    image = {"n_pred": ka, "n_gt": kb, "n_merged": sum(1 for r in pred if r[2] >= 2), "n_split": sum(1 for r in gt if r[2] >= 2),
             "n_missed": kb - len(seen_b), "n_spurious": ka - len(seen_a)}
    for k in range(10, 20):
        image[f"tp_{5 * k}"] = tp[k]
    image.update(inter_px=inter, pred_px=sum(area_a), gt_px=sum(area_b))
    return [tuple(r) for r in pred], [tuple(r) for r in gt], image


def ratios_ref(image):
    """The float columns of the per-image row from its integers."""
    ka, kb = image["n_pred"], image["n_gt"]

    def ratio(num, den):
        if ka == 0 and kb == 0:
            return 1.0
        return num / den if den != 0 else 0.0
    tp = image["tp_50"]
    out = {"precision_50": ratio(tp, ka), "recall_50": ratio(tp, kb), "f1_50": ratio(2 * tp, ka + kb)}
    total = 0.0
    for k in range(10, 20):
        t = image[f"tp_{5 * k}"]
        out[f"ap_{5 * k}"] = ratio(t, ka + kb - t)
        total += out[f"ap_{5 * k}"]
    out["mean_ap"] = total / 10
    px = image["pred_px"] + image["gt_px"]
    out["pixel_dice"] = ratio(2 * image["inter_px"], px)
    out["pixel_iou"] = ratio(image["inter_px"], px - image["inter_px"])
    return out
