"""The lesion matching restated from its definition, for the tests: scipy.ndimage.label with the full 3 x 3 x 3
neighbourhood on both masks, numpy.unique over the (label id, predicted id) of the voxels both hold, and the scores
through the dense overlap matrix in exact fractions.  Nothing here is shared with efficientq_amd.lesion_match."""
from fractions import Fraction

import numpy as np
from scipy import ndimage

FULL = np.ones((3, 3, 3), np.int64)


def ref_pairs(pred, gt):
    """(label sizes, predicted sizes, pairs n x 3 int64 = label row, predicted row, common voxels), rows 0-based in
    scipy's numbering, pairs ascending in (label row, predicted row)."""
    lp, n_p = ndimage.label(np.asarray(pred) != 0, structure=FULL)
    ll, n_l = ndimage.label(np.asarray(gt) != 0, structure=FULL)
    a = np.bincount(ll.ravel(), minlength=n_l + 1)[1:].astype(np.int64)
    b = np.bincount(lp.ravel(), minlength=n_p + 1)[1:].astype(np.int64)
    both = (lp > 0) & (ll > 0)
    ids = np.stack([ll[both], lp[both]], 1).astype(np.int64).reshape(-1, 2)
    if len(ids) == 0:
        return a, b, np.zeros((0, 3), np.int64)
    keys, counts = np.unique(ids, axis=0, return_counts=True)       # sorted by label id, then predicted id
    return a, b, np.concatenate([keys - 1, counts[:, None].astype(np.int64)], 1)


def ref_scores(a, b, pairs):
    """The scores of one class from the dense overlap matrix, as exact fractions turned into floats at the end."""
    nl, npred = len(a), len(b)
    n = np.zeros((nl, npred), dtype=object)
    n[...] = 0
    for i, j, v in np.asarray(pairs, np.int64).reshape(-1, 3).tolist():
        n[i, j] = int(v)
    iou = [[Fraction(n[i, j], int(a[i]) + int(b[j]) - n[i, j]) for j in range(npred)] for i in range(nl)]
    matches = [(i, j) for i in range(nl) for j in range(npred) if iou[i][j] > Fraction(1, 2)]
    tp = len(matches)
    fn, fp = nl - tp, npred - tp
    lab = {"match": [0] * nl, "best_iou": [0.0] * nl, "partners": [0] * nl}
    prd = {"match": [0] * npred, "best_iou": [0.0] * npred, "partners": [0] * npred}
    for i, j in matches:
        assert lab["match"][i] == 0 and prd["match"][j] == 0, "a lesion in two matches"
        lab["match"][i], prd["match"][j] = j + 1, i + 1
    for i in range(nl):
        lab["partners"][i] = sum(1 for j in range(npred) if n[i, j] > 0)
        lab["best_iou"][i] = float(max(iou[i], default=Fraction(0)))
    for j in range(npred):
        prd["partners"][j] = sum(1 for i in range(nl) if n[i, j] > 0)
        prd["best_iou"][j] = float(max((iou[i][j] for i in range(nl)), default=Fraction(0)))
    out = {"tp_l": tp, "fp_l": fp, "fn_l": fn, "label": lab, "pred": prd, "matches": matches}
    if nl + npred == 0:
        out.update(groups=0, f1_l=1.0, sq=1.0, pq=1.0, lw_dsc=1.0, group_sets=[])
        return out
    # the groups: flood the bipartite graph whose edges are the non-zero overlaps
    seen_l, seen_p, groups = set(), set(), []
    for i0 in range(nl):
        if i0 in seen_l or lab["partners"][i0] == 0:
            continue
        gl, gp, todo = {i0}, set(), [("l", i0)]
        while todo:
            side, k = todo.pop()
            if side == "l":
                for j in range(npred):
                    if n[k, j] > 0 and j not in gp:
                        gp.add(j)
                        todo.append(("p", j))
            else:
                for i in range(nl):
                    if n[i, k] > 0 and i not in gl:
                        gl.add(i)
                        todo.append(("l", i))
        seen_l |= gl
        seen_p |= gp
        groups.append((sorted(gl), sorted(gp)))
    scores = [Fraction(2 * sum(n[i, j] for i in gl for j in gp), sum(int(a[i]) for i in gl) + sum(int(b[j]) for j in gp))
              for gl, gp in groups]
    loose = sum(1 for i in range(nl) if lab["partners"][i] == 0) + sum(1 for j in range(npred) if prd["partners"][j] == 0)
    siou = sum((iou[i][j] for i, j in matches), Fraction(0))
    out.update(groups=len(groups), group_sets=groups, f1_l=float(Fraction(2 * tp, 2 * tp + fp + fn)),
               sq=float(siou / tp) if tp else 0.0, pq=float(siou / (Fraction(tp) + Fraction(fp, 2) + Fraction(fn, 2))),
               lw_dsc=float(sum(scores, Fraction(0)) / (len(groups) + loose)))
    return out
