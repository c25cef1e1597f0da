"""Lesion-wise scores of one class from the sizes of its label lesions and predicted lesions and the overlap of every pair
of them (ops_match.seg_lesion_match): one-to-one matching at IoU > 0.5, lesion F1, segmentation and panoptic quality,
and a lesion-wise Dice over the groups of overlapping lesions.  Pure numpy on the host: every decision is taken on exact
integers, the scores are fp64 quotients of them.

Lesions i (label, size a_i) and j (predicted, size b_j) with n_ij common voxels match when
IoU_ij = n_ij / (a_i + b_j - n_ij) > 1/2, decided as 3 n_ij > a_i + b_j.  The inequality is strict, and that makes the
matching one to one: two partners j, j' of one lesion i are disjoint, so n_ij + n_ij' <= a_i, while 3 n_ij > a_i + b_j >=
a_i + n_ij gives n_ij > a_i / 2 for both.  With >= it is not: a label lesion of two voxels whose voxels are two predicted
lesions of one voxel each has IoU 1/2 with both."""
from __future__ import annotations

import numpy as np

MATCH_COLUMNS = ("tp_l", "fp_l", "fn_l", "f1_l", "sq", "pq", "lw_dsc", "groups")     # lesion_match.csv, after subject, class
PAIR_COLUMNS = ("label_lesion", "pred_lesion", "overlap", "iou")                      # lesion_pairs.csv, after subject, class
LESION_COLUMNS = ("match", "best_iou", "partners")                                    # lesions.csv gains these, last
SCORES = ("f1_l", "sq", "pq", "lw_dsc")


def _side(n: int, own, other, iou, matched):
    """match (1-based number of the partner, 0: none), best_iou and partners of the n lesions of one mask; own / other:
    their 0-based rows and their partners' in every pair."""
    match = np.zeros(n, np.int64)
    best = np.zeros(n, np.float64)
    match[own[matched]] = other[matched] + 1
    np.maximum.at(best, own, iou)
    return {"match": match, "best_iou": best, "partners": np.bincount(own, minlength=n).astype(np.int64)}


def _groups(nl: int, npred: int, li, pj):
    """Union-find over the pairs: the root of every node, label lesion i = node i, predicted lesion j = node nl + j."""
    parent = list(range(nl + npred))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for i, j in zip(li.tolist(), pj.tolist()):
        a, b = find(i), find(nl + j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(nl + npred)], np.int64)


def match_class(label_sizes, pred_sizes, pairs) -> dict:
    """The scores of one class.  label_sizes (nl), pred_sizes (np): voxels per lesion, in the order of their rows; pairs
    (n x 3): label row, predicted row (0-based), common voxels > 0, every pair once.  Returns tp_l, fp_l, fn_l, groups
    (int), f1_l, sq, pq, lw_dsc (float), iou (n) fp64 and matched (n) bool per pair in the order given, and "label" /
    "pred": match, best_iou, partners and group (the 1-based number of the lesion's group of lw_dsc, in ascending order
    of the group's first label lesion; 0: it shares no voxel) per lesion.  A class without any lesion: the counts 0, the
    four scores 1."""
    a = np.asarray(label_sizes, np.int64).reshape(-1)
    b = np.asarray(pred_sizes, np.int64).reshape(-1)
    pr = np.asarray(pairs, np.int64).reshape(-1, 3)
    li, pj, n = pr[:, 0], pr[:, 1], pr[:, 2]
    nl, npred = len(a), len(b)
    if len(pr) and (li.min() < 0 or li.max() >= nl or pj.min() < 0 or pj.max() >= npred or n.min() <= 0):
        raise ValueError("match_class: a pair names a lesion that is not there, or has no voxel")
    tot = a[li] + b[pj]
    matched = 3 * n > tot                                   # IoU > 1/2, in integers
    iou = n / (tot - n).astype(np.float64) if len(pr) else np.zeros(0, np.float64)
    tp = int(matched.sum())
    if tp != len(set(li[matched].tolist())) or tp != len(set(pj[matched].tolist())):
        raise ValueError("match_class: a lesion in two matches: the pairs or the sizes are not those of two labellings")
    fn, fp = nl - tp, npred - tp
    out = {"tp_l": tp, "fp_l": fp, "fn_l": fn, "iou": iou, "matched": matched,
           "label": _side(nl, li, pj, iou, matched), "pred": _side(npred, pj, li, iou, matched)}
    out["label"]["group"], out["pred"]["group"] = np.zeros(nl, np.int64), np.zeros(npred, np.int64)
    if nl + npred == 0:
        out.update(groups=0, f1_l=1.0, sq=1.0, pq=1.0, lw_dsc=1.0)
        return out
    root = _groups(nl, npred, li, pj)
    groot = np.unique(root[li])                             # the groups: the components that hold a pair
    gi = np.searchsorted(groot, root[li])
    num = np.zeros(len(groot), np.int64)
    den = np.zeros(len(groot), np.int64)
    np.add.at(num, gi, 2 * n)
    paired_l = np.bincount(li, minlength=nl) > 0
    paired_p = np.bincount(pj, minlength=npred) > 0
    np.add.at(den, np.searchsorted(groot, root[:nl][paired_l]), a[paired_l])
    np.add.at(den, np.searchsorted(groot, root[nl:][paired_p]), b[paired_p])
    out["label"]["group"][paired_l] = np.searchsorted(groot, root[:nl][paired_l]) + 1
    out["pred"]["group"][paired_p] = np.searchsorted(groot, root[nl:][paired_p]) + 1
    loose = int((~paired_l).sum()) + int((~paired_p).sum())
    siou = float(iou[matched].sum())
    out.update(groups=int(len(groot)), f1_l=2 * tp / (2 * tp + fp + fn), sq=siou / tp if tp else 0.0,
               pq=siou / (tp + fp / 2 + fn / 2), lw_dsc=float((num / den.astype(np.float64)).sum()) / (len(groot) + loose))
    return out


def case_scores(rows, pairs) -> list:
    """match_class for every class of one case from what ops_match.seg_lesion_match returns: rows, 2 C tables n x 3
    (first voxel, size, overlap; plane c predicted, plane C + c label) and pairs, C tables n x 3.  Each dict also carries
    "pairs", the int64 n x 3 pairs themselves."""
    ncls = len(pairs)
    out = []
    for c in range(ncls):
        pr = np.asarray(pairs[c], np.int64).reshape(-1, 3)
        res = match_class(np.asarray(rows[ncls + c], np.int64).reshape(-1, 3)[:, 1],
                          np.asarray(rows[c], np.int64).reshape(-1, 3)[:, 1], pr)
        res["pairs"] = pr
        out.append(res)
    return out


def _fmt(v) -> str:
    return "%.7g" % float(v)


def write_lesion_match_csv(path: str, results) -> None:
    """One row per subject and class of results that carry "lesion_match" (validate_seg(..., lesion_match=True)):
    subject, class and MATCH_COLUMNS."""
    import csv
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + MATCH_COLUMNS)
        for r in results:
            for c, m in enumerate(r.get("lesion_match", ())):
                wr.writerow([r["name"], c, m["tp_l"], m["fp_l"], m["fn_l"]] + [_fmt(m[k]) for k in SCORES] + [m["groups"]])


def write_lesion_pairs_csv(path: str, results) -> None:
    """One row per pair of overlapping lesions of results that carry "lesion_match": subject, class, label_lesion,
    pred_lesion (1-based, the numbers of lesions.csv), overlap in voxels, iou; ascending in (label_lesion, pred_lesion)
    per subject and class."""
    import csv
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + PAIR_COLUMNS)
        for r in results:
            for c, m in enumerate(r.get("lesion_match", ())):
                for (i, j, n), q in zip(m["pairs"].tolist(), m["iou"].tolist()):
                    wr.writerow([r["name"], c, i + 1, j + 1, n, _fmt(q)])


def match_summary(results) -> list:
    """Per class over the cases that carry "lesion_match": the mean f1_l, pq and lw_dsc and the pooled tp_l, fp_l, fn_l."""
    res = [r["lesion_match"] for r in results if "lesion_match" in r]
    out = []
    for c in range(max((len(m) for m in res), default=0)):
        per = [m[c] for m in res if c < len(m)]
        row = {k: float(np.mean([m[k] for m in per])) for k in ("f1_l", "pq", "lw_dsc")}
        row.update({k: int(sum(m[k] for m in per)) for k in ("tp_l", "fp_l", "fn_l")})
        out.append(row)
    return out
