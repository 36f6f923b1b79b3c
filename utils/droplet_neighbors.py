"""Droplet neighbourhoods of a label map on the host (numpy + scipy, no torch): contact pairs, nearest contact, degree and
cluster per droplet.  The definition is DESIGN.md section 20; this module is the CPU path of quantify_droplets_batch.py
--neighbors and the yardstick of csrc/neighbors.hip.  Everything is integer work: the squared distances are rebuilt from the
integer indices of the distance transform, never from its float distances."""
from __future__ import annotations

import numpy as np

EDT_INF = 2 ** 31 - 1       # UNETDC_EDT_INF
DEFAULT_RADIUS = 5          # pixels: a convention of the command line, not a measured number
MAX_RADIUS = 64
COLUMN_NAMES = ("nn_label", "nn_d2", "degree", "cluster", "cluster_size")


def check_radius(G):
    """-> G as int; ValueError for what unetdc_label_neighbors refuses (an integer 1..64)."""
    if isinstance(G, bool) or not isinstance(G, (int, np.integer)) or not 1 <= int(G) <= MAX_RADIUS:
        raise ValueError(f"the contact radius must be an integer in 1..{MAX_RADIUS} pixels, not {G!r}")
    return int(G)


def in_range(label, max_label):
    """The label map with every value below 1 or above max_label set to 0, int64."""
    lab = np.asarray(label).astype(np.int64)
    return np.where((lab >= 1) & (lab <= int(max_label)), lab, 0)


def neighbor_pairs_numpy(label, max_label, G):
    """-> (a, b, d2) int64 arrays: the pairs a < b with d2 <= G * G, in ascending order of (a, b).  Per label one distance
    transform of "not this label" in the window of its bounding box grown by G (which holds every pixel within G of it)."""
    from scipy import ndimage
    G = check_radius(G)
    lab = in_range(label, max_label)
    h, w = lab.shape
    out_a, out_b, out_d = [], [], []
    for k, sl in enumerate(ndimage.find_objects(lab.astype(np.int32), int(max_label)), start=1):
        if sl is None:
            continue
        y0, y1 = max(sl[0].start - G, 0), min(sl[0].stop + G, h)
        x0, x1 = max(sl[1].start - G, 0), min(sl[1].stop + G, w)
        sub = lab[y0:y1, x0:x1]
        others = np.unique(sub[sub > k])
        if others.size == 0:
            continue
        iy, ix = ndimage.distance_transform_edt(sub != k, return_distances=False, return_indices=True)
        yy, xx = np.mgrid[0:sub.shape[0], 0:sub.shape[1]]
        d2 = (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2
        dmin = np.asarray(ndimage.minimum(d2, sub, index=others)).astype(np.int64).reshape(-1)
        keep = dmin <= G * G
        out_a.append(np.full(int(keep.sum()), k, np.int64))
        out_b.append(others[keep])
        out_d.append(dmin[keep])
    if not out_a:
        return tuple(np.zeros(0, np.int64) for _ in range(3))
    return np.concatenate(out_a), np.concatenate(out_b), np.concatenate(out_d)


def present_labels(label, max_label):
    """bool [max_label]: entry k - 1 says whether label k has a pixel."""
    return np.bincount(in_range(label, max_label).ravel(), minlength=int(max_label) + 1)[1:] > 0


def neighbor_columns(pairs, K, present=None):
    """pairs (a, b, d2) as above, K labels -> the five per-label int64 arrays of COLUMN_NAMES, entry k - 1 for label k.
    present (bool [K], None = every label has a pixel) only enters cluster_size."""
    a, b, d2 = (np.asarray(v, dtype=np.int64) for v in pairs)
    K = int(K)
    present = np.ones(K, bool) if present is None else np.asarray(present, dtype=bool)
    ends = np.concatenate([a, b]) - 1
    other = np.concatenate([b, a])
    dist = np.concatenate([d2, d2])
    degree = np.bincount(ends, minlength=K).astype(np.int64)
    nn_label, nn_d2 = np.zeros(K, np.int64), np.full(K, EDT_INF, np.int64)
    order = np.lexsort((other, dist, ends))[::-1]            # the last write per label is its smallest (d2, other)
    nn_label[ends[order]] = other[order]
    nn_d2[ends[order]] = dist[order]
    cluster = np.arange(1, K + 1, dtype=np.int64)
    if K and a.size:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _, comp = connected_components(coo_matrix((np.ones(a.size, np.int8), (a - 1, b - 1)), shape=(K, K)), directed=False)
        first = np.full(comp.max() + 1, K + 1, np.int64)
        np.minimum.at(first, comp, cluster)
        cluster = first[comp]
    members = np.bincount(cluster[present] - 1, minlength=K).astype(np.int64)
    size = np.where(present, members[cluster - 1], 0) if K else np.zeros(0, np.int64)
    return dict(zip(COLUMN_NAMES, (nn_label, nn_d2, degree, cluster, size)))


def neighbors_numpy(label, max_label, G):
    """The record of Droplets.neighbors from a host label map: {"pairs": {"a", "b", "d2"}, and the five columns}."""
    pairs = neighbor_pairs_numpy(label, max_label, G)
    return {"pairs": dict(zip("a b d2".split(), pairs)), **neighbor_columns(pairs, max_label, present_labels(label, max_label))}


SUMMARY_NAMES = ("n_contacts", "n_clusters", "n_clustered", "n_isolated", "largest_cluster", "mean_nn_dist_px", "n_touching")


def summary(pairs, columns):
    """One image's numbers: contact pairs, clusters of two or more, droplets in them, droplets alone, the largest cluster,
    the mean nearest-contact distance in pixels over the droplets that have one (NaN without any), pairs with d2 <= 2."""
    d2 = np.asarray(pairs[2], dtype=np.int64)
    size, cluster, nn = (np.asarray(columns[q], dtype=np.int64) for q in ("cluster_size", "cluster", "nn_d2"))
    clustered = size >= 2
    has = nn != EDT_INF
    return {"n_contacts": int(d2.size), "n_clusters": int(np.unique(cluster[clustered]).size), "n_clustered": int(clustered.sum()),
            "n_isolated": int((size == 1).sum()), "largest_cluster": int(size.max(initial=0)),
            "mean_nn_dist_px": float(np.sqrt(nn[has].astype(np.float64)).mean()) if has.any() else float("nan"),
            "n_touching": int((d2 <= 2).sum())}


def table_columns(rec, centroid_row, centroid_col, px_per_um=None):
    """The columns --neighbors adds to a droplet table, from the record of neighbors_numpy and the table's centroids:
    nn_label (0 without a contact), nn_dist_px = sqrt(nn_d2) and nn_centroid_dist_px (both NaN without a contact),
    n_contacts, cluster, cluster_size, and nn_dist_micron given pixels per micron."""
    nn, d2 = np.asarray(rec["nn_label"], dtype=np.int64), np.asarray(rec["nn_d2"], dtype=np.int64)
    cy, cx = np.asarray(centroid_row, dtype=np.float64), np.asarray(centroid_col, dtype=np.float64)
    has = nn > 0
    j = np.where(has, nn - 1, 0)
    dist = np.where(has, np.sqrt(np.where(has, d2, 0).astype(np.float64)), np.nan)
    cen = np.where(has, np.sqrt((cy[j] - cy) ** 2 + (cx[j] - cx) ** 2), np.nan) if nn.size else np.zeros(0)
    out = {"nn_label": nn, "nn_dist_px": dist, "nn_centroid_dist_px": cen, "n_contacts": np.asarray(rec["degree"], dtype=np.int64),
           "cluster": np.asarray(rec["cluster"], dtype=np.int64), "cluster_size": np.asarray(rec["cluster_size"], dtype=np.int64)}
    if px_per_um is not None:
        out["nn_dist_micron"] = dist / px_per_um
    return out


def contact_table(filename, pairs):
    """One image's rows of droplet_contacts.csv, in (a, b) order."""
    a, b, d2 = (np.asarray(v, dtype=np.int64) for v in pairs)
    return {"filename": [filename] * a.size, "label_a": a, "label_b": b, "d2": d2, "dist_px": np.sqrt(d2.astype(np.float64))}
