"""The host arithmetic of the validation over counts and results: Dice of hard predictions (``utils/metrics.py:21-45,
119-148``), the metrics of confusion counts, the surface distances from what the device returns, the threshold sweep
(AUC, best threshold) and the means and totals over the cases.  No device and no file.  evaluate.py imports every name:
``evaluate.X`` is the object defined here."""
from __future__ import annotations

import math

import numpy as np
import torch

METRICS = ("dsc", "sens", "spec", "acc")
EPS = 1e-6                # metrics.py
LESION_COLUMNS = ("totall", "predl", "fnl", "fpl")     # the columns of "lesions" (hip_ops.seg_lesions)
LESION_TABLE_COLUMNS = ("d", "h", "w", "size", "overlap")   # the columns of "lesion_table" (hip_ops.seg_lesion_table)
LESION_SIZE_BINS = ((1, 9), (10, 99), (100, 999), (1000, None))    # lesion_size_summary: voxels, both ends included
SURFACE_COLUMNS = ("hd", "hd95", "assd")               # the columns of "surface" (surface_metrics), voxel units
SURFACE_COLUMNS_MM = ("hd_mm", "hd95_mm", "assd_mm")   # the same in millimetres (surface_metrics_mm)
AGREEMENT_COUNTS = ("both", "q_only", "fp_only", "neither")          # the columns of "vs_fp"'s counts
AGREEMENT_DRIFT = ("logit_rel_mse", "logit_max", "prob_mae")        # the per-class drift entries of "vs_fp"


def dice(pred_b: torch.Tensor, target_b: torch.Tensor) -> torch.Tensor:
    """metrics.py:21-25."""
    eps = 1e-6
    return (2 * (pred_b * target_b).sum().float() + eps) / (pred_b.sum().float() + target_b.sum().float() + eps)


def validate_vs_label(output: torch.Tensor, target: torch.Tensor, task: str = "lits"):
    """Dice of the hard predictions of `output` (NCDHW logits, or M x NCDHW for M heads) against `target`
    (metrics.py:119-148): per class for lits, background + per channel for brats."""
    if output.dim() >= 6:
        return [validate_vs_label(o, target, task) for o in output]
    if task == "lits":
        pred = torch.max(output, 1)[1]
        return [dice(pred == c, target == c) for c in range(output.shape[1])]
    if task == "brats":
        pred = (torch.sigmoid(output) >= 0.5).int()
        m = [dice(pred.sum(dim=1) == 0, target.sum(dim=1) == 0)]
        return m + [dice(pred[:, c], target[:, c]) for c in range(output.shape[1])]
    raise RuntimeError(f"Unknown task {task}")


def metrics_from_counts(counts: torch.Tensor) -> dict:
    """dice / sensitivity / specificity / accuracy per class from C x 4 counts (TP, FP, FN, TN), in the fp32
    arithmetic of metrics.py:21-45 on those same integer sums (eps included)."""
    counts = counts.to("cpu", torch.int64)
    tp, fp, fn, tn = counts.unbind(1)
    n = torch.tensor(float(counts[0].sum()), dtype=torch.float)
    return {"dsc": (2 * tp.float() + EPS) / ((tp + fp).float() + (tp + fn).float() + EPS),
            "sens": (tp.float() + EPS) / ((tp + fn).float() + EPS),
            "spec": (tn.float() + EPS) / ((tn + fp).float() + EPS),
            "acc": (tp + tn).float() / n}


def _surface_rows(rows, diag: float) -> torch.Tensor:
    """hd, hd95, assd per class (C x 3 float64) from one (n_p, n_l, max_sq, qlo_sq, qhi_sq, sum_pl, sum_lp) per class -
    the two surface counts, the largest squared distance, the two pooled order statistics squared and the two directed
    sums - and the diagonal that stands for a distance to an empty surface: the formulas of surface_metrics."""
    out = torch.zeros(len(rows), 3, dtype=torch.float64)
    for c, (n_p, n_l, max_sq, qlo, qhi, sum_pl, sum_lp) in enumerate(rows):
        if n_p == 0 and n_l == 0:
            continue
        if n_p == 0 or n_l == 0:
            out[c] = diag
            continue
        r = 95 * (n_p + n_l - 1) % 100
        lo, hi = math.sqrt(qlo), math.sqrt(qhi)
        out[c, 0] = math.sqrt(max_sq)
        out[c, 1] = lo + (hi - lo) * r / 100
        out[c, 2] = (sum_pl / n_p + sum_lp / n_l) / 2
    return out


def surface_metrics(counts, sums, shape) -> torch.Tensor:
    """hd, hd95, assd per class (C x 3 float64, voxel units) of one case of extent `shape` = (D, H, W) from what
    hip_ops.seg_surface returns: counts C x 6 = nP, nL, maxsq_PL, maxsq_LP, qlo_sq, qhi_sq and sums C x 2.  With the
    surface voxels S(P), S(L) of the predicted and the label mask and the distances of each to the other surface:
    hd = the largest of all, hd95 = the 95th percentile of the n = nP + nL pooled distances with linear interpolation
    between the order statistics (numpy.percentile: 95 (n - 1) = 100 lo + r in integers, v[lo] + (v[min(lo + 1, n - 1)]
    - v[lo]) r / 100), assd = the mean of the two directed means: medpy's hd, hd95 and assd.  Both surfaces empty: 0;
    one of them empty: sqrt(D^2 + H^2 + W^2) for all three (the BraTS convention)."""
    counts = torch.as_tensor(counts).to("cpu", torch.int64)
    sums = torch.as_tensor(sums).to("cpu", torch.float64)
    diag = math.sqrt(sum(int(e) ** 2 for e in shape))
    rows = [(n_p, n_l, max(max_pl, max_lp), qlo, qhi, *s)                   # the squares stay Python ints: sqrt is exact
            for (n_p, n_l, max_pl, max_lp, qlo, qhi), s in zip(counts.tolist(), sums.tolist())]
    return _surface_rows(rows, diag)


def surface_metrics_mm(counts, sq, sums, shape, spacing) -> torch.Tensor:
    """hd, hd95, assd per class (C x 3 float64, millimetres) of one case of extent `shape` = (D, H, W) on a grid of
    `spacing` = (d, h, w) mm from what hip_ops.seg_surface_mm returns: counts C x 2 = nP, nL, sq C x 4 fp32 = max_PL,
    max_LP, qlo, qhi (mm^2) and sums C x 2.  The definitions are surface_metrics': hd = sqrt of the larger maximum,
    hd95 = the same interpolation between sqrt(qlo) and sqrt(qhi), assd = the mean of the two directed means.  Both
    surfaces empty: 0; one of them empty: the physical diagonal sqrt(sum_a (extent_a spacing_a)^2) for all three."""
    counts = torch.as_tensor(counts).to("cpu", torch.int64)
    sq = torch.as_tensor(sq).to("cpu", torch.float64)
    sums = torch.as_tensor(sums).to("cpu", torch.float64)
    diag = math.sqrt(sum((int(e) * float(s)) ** 2 for e, s in zip(shape, spacing)))
    rows = [(*n, max(max_pl, max_lp), qlo, qhi, *s)
            for n, (max_pl, max_lp, qlo, qhi), s in zip(counts.tolist(), sq.tolist(), sums.tolist())]
    return _surface_rows(rows, diag)


# ---- the threshold sweep (validate_seg(..., sweep=True), --thr_sweep) -----------------------------------------------------
SWEEP_BINS = 4096
SWEEP_MID = 2048          # the edge of the default decision: row 2048 of a sweep is the counts of metrics.csv


def _sweep_ints(hist):
    """A histogram (tensor, array or nested lists; C x 2 x 4096) as nested lists of Python integers."""
    if hasattr(hist, "tolist"):
        hist = hist.tolist()
    out = [[[int(v) for v in row] for row in cls] for cls in hist]
    if any(len(cls) != 2 or any(len(row) != SWEEP_BINS for row in cls) for cls in out):
        raise ValueError(f"a sweep histogram is C x 2 x {SWEEP_BINS}")
    return out


def sweep_pooled(hists):
    """The sum of histograms (each C x 2 x 4096) in Python integers, as nested lists."""
    hs = [_sweep_ints(h) for h in hists]
    return [[[sum(col) for col in zip(*(h[c][g] for h in hs))] for g in range(2)] for c in range(len(hs[0]))]


def sweep_summary(hist, edges):
    """Per class of a sweep histogram (C x 2 x 4096: [c][g][b] = the voxels of truth g in score bin b; hip_ops.seg_sweep, or
    sweep_pooled of several) and the 4096 edges of its bins, on the host and in integers, a dict of
      auc          (2 sum_b pos_b below_b + sum_b pos_b neg_b) / (2 P N), below_b = the negatives in the bins under b: the
                   Mann-Whitney statistic with the ties inside a bin counted half (roc_auc_score(truth, bin)); the
                   numerator is an exact Python integer; 1.0 when P = 0 or N = 0 (metrics.py:60-67)
      counts       4096 x 4 int64, row k = TP, FP, FN, TN of the decision "score >= edge k" (suffix sums; row 0: all)
      best_k       the k in 1 .. 4095 with the largest 2 TP / (2 TP + FP + FN) in fp64 (a zero denominator counts as -1);
                   ties go to the least |k - 2048|, then to the lower k
      best_thr     edge best_k as a Python float (an fp32 value)
      dsc_default, dsc_best, sens_best, spec_best    metrics_from_counts of the rows 2048 and best_k (the arithmetic of
                   metrics.csv)
      pos, neg     P and N."""
    h = _sweep_ints(hist)
    e = [float(v) for v in (edges.tolist() if hasattr(edges, "tolist") else edges)]
    if len(e) != SWEEP_BINS:
        raise ValueError(f"{len(e)} edges, a sweep has {SWEEP_BINS}")
    out = []
    for neg, pos in h:
        P, N = sum(pos), sum(neg)
        num, below = 0, 0
        for pb, nb in zip(pos, neg):
            num += 2 * pb * below + pb * nb
            below += nb
        auc = num / (2 * P * N) if P and N else 1.0
        rows, tp, fp = [None] * SWEEP_BINS, 0, 0
        for k in range(SWEEP_BINS - 1, -1, -1):
            tp += pos[k]
            fp += neg[k]
            rows[k] = (tp, fp, P - tp, N - fp)
        best_k, best = None, None
        for k in range(1, SWEEP_BINS):
            tp, fp, fn, _ = rows[k]
            den = 2 * tp + fp + fn
            key = ((2 * tp) / den if den else -1.0, -abs(k - SWEEP_MID), -k)
            if best is None or key > best:
                best_k, best = k, key
        counts = torch.tensor(rows, dtype=torch.int64)
        m = metrics_from_counts(counts[[SWEEP_MID, best_k]])
        out.append({"auc": auc, "counts": counts, "best_k": best_k, "best_thr": e[best_k],
                    "dsc_default": m["dsc"][0], "dsc_best": m["dsc"][1], "sens_best": m["sens"][1],
                    "spec_best": m["spec"][1], "pos": P, "neg": N})
    return out


def logit_prob(logit: float) -> float:
    """1 / (1 + exp(-logit)) in fp64."""
    return 1.0 / (1.0 + math.exp(-logit))


def sweep_results(results):
    """(per-subject [(name, summary)], pooled summary, edges) of the results that carry "sweep"."""
    res = [r for r in results if "sweep" in r]
    if not res:
        raise RuntimeError("no result carries a sweep (validate_seg(..., sweep=True) on labelled cases)")
    edges = res[0]["sweep_edges"]
    if any(not torch.equal(torch.as_tensor(r["sweep_edges"]), torch.as_tensor(edges)) for r in res):
        raise RuntimeError("sweeps with different edges in one file")
    per = [(r["name"], sweep_summary(r["sweep"], edges)) for r in res]
    return per, sweep_summary(sweep_pooled([r["sweep"] for r in res]), edges), edges


def post_means(results) -> dict:
    """Per-class mean of dsc / sens / spec / acc over the "post" entries."""
    return {m: torch.stack([r["post"][m] for r in results if "post" in r]).mean(0) for m in METRICS}


def agreement_means(results) -> dict:
    """Means over the cases of the "vs_fp" entries: dsc, logit_rel_mse and prob_mae per class, and flip_frac."""
    vs = [r["vs_fp"] for r in results if "vs_fp" in r]
    out = {k: torch.stack([v[k].to(torch.float64) for v in vs]).mean(0) for k in ("dsc", "logit_rel_mse", "prob_mae")}
    out["flip_frac"] = sum(v["flip_frac"] for v in vs) / len(vs)
    return out


def lesion_size_summary(results) -> np.ndarray:
    """The label lesions of results that carry "lesion_table" per class and size bin (LESION_SIZE_BINS: 1-9, 10-99,
    100-999, >= 1000 voxels): C x 4 x 2 int64 = the lesions of the bin over all cases, and how many of them were
    detected (overlap > 0)."""
    res = [r for r in results if "lesion_table" in r]
    out = np.zeros((max((len(r["lesion_table"]) for r in res), default=0), len(LESION_SIZE_BINS), 2), np.int64)
    for r in res:
        for c, (label_rows, _) in enumerate(r["lesion_table"]):
            rows = np.asarray(label_rows, dtype=np.int64).reshape(-1, 5)
            for b, (lo, hi) in enumerate(LESION_SIZE_BINS):
                sel = (rows[:, 3] >= lo) & ((rows[:, 3] <= hi) if hi is not None else True)
                out[c, b, 0] += int(sel.sum())
                out[c, b, 1] += int((sel & (rows[:, 4] > 0)).sum())
    return out


def metric_means(results) -> dict:
    """Per-class mean over the cases of each metric."""
    return {m: torch.stack([r[m] for r in results]).mean(0) for m in METRICS}


def lesion_totals(results) -> torch.Tensor:
    """Per-class sums over the cases of the lesion-level counts (C x 4 int64: LESION_COLUMNS)."""
    return torch.stack([r["lesions"].to("cpu", torch.int64) for r in results]).sum(0)


def surface_means(results) -> torch.Tensor:
    """Per-class means over the cases of the surface distances (C x 3 float64: SURFACE_COLUMNS)."""
    return torch.stack([r["surface"].to("cpu", torch.float64) for r in results]).mean(0)
