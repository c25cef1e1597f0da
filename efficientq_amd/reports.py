"""The reports of a validation: the CSV files written from validate_seg's results (``metrics.csv``, ``threshold.csv``,
``threshold_curve.csv``, ``metrics_post.csv``, ``agreement.csv``, ``lesions.csv``) and the lines the ``ptq`` mission
prints about them (the ``*_lines`` functions return the lines; entrance._ValidationTester prints them).  The writers of
``--lesion_match`` stay in lesion_match.py.  evaluate.py imports every name: ``evaluate.X`` is the object defined here."""
from __future__ import annotations

import csv

import numpy as np
import torch

from .metrics import (AGREEMENT_COUNTS, AGREEMENT_DRIFT, LESION_COLUMNS, LESION_SIZE_BINS, LESION_TABLE_COLUMNS, METRICS,
                      SURFACE_COLUMNS, SURFACE_COLUMNS_MM, SWEEP_BINS, agreement_means, lesion_size_summary,
                      lesion_totals, logit_prob, metric_means, metrics_from_counts, post_means, surface_means,
                      sweep_results)


def _lesion_surface_columns(entries, who: str):
    """(the columns, a function (entry, class) -> their values) of the optional lesion counts and surface distances of
    `entries`: hd, hd95, assd, named hd_mm, hd95_mm, assd_mm when the entries are in millimetres ("surface_unit")."""
    cc = any("lesions" in v for v in entries)
    sd = any("surface" in v for v in entries)
    units = {v.get("surface_unit", "voxel") for v in entries if "surface" in v}
    if len(units) > 1:
        raise RuntimeError(f"{who}: surface distances in voxel units and in mm in one file")
    cols = (LESION_COLUMNS if cc else ()) + ((SURFACE_COLUMNS_MM if units == {"mm"} else SURFACE_COLUMNS) if sd else ())
    return cols, lambda v, c: ([int(n) for n in v["lesions"][c]] if cc else []) + \
        (["%.7g" % float(n) for n in v["surface"][c]] if sd else [])


def write_metrics_csv(path: str, results) -> None:
    """One row per subject and class: subject, class, dsc, sens, spec, acc, tp, fp, fn, tn, and when the results carry
    "lesions" (validate_seg(..., lesions=True)) also totall, predl, fnl, fpl, and when they carry "surface"
    (validate_seg(..., surface=True)) after those hd, hd95, assd - named hd_mm, hd95_mm, assd_mm when the results are in
    millimetres ("surface_unit": validate_seg(..., geometry=...)); a file never mixes the two."""
    cols, values = _lesion_surface_columns(results, "write_metrics_csv")
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + METRICS + ("tp", "fp", "fn", "tn") + cols)
        for r in results:
            for c in range(r["counts"].shape[0]):
                wr.writerow([r["name"], c] + ["%.7g" % float(r[m][c]) for m in METRICS] +
                            [int(v) for v in r["counts"][c]] + values(r, c))


THRESHOLD_COLUMNS = ("subject", "class", "auc", "dsc", "best_thr_logit", "best_thr_prob", "dsc_best", "sens_best",
                     "spec_best", "pos", "neg")
THRESHOLD_CURVE_COLUMNS = ("class", "k", "thr_logit", "thr_prob", "tp", "fp", "fn", "tn", "dsc", "sens", "spec")


def write_threshold_csv(path: str, results) -> None:
    """One row per subject and class from the "sweep" entries (validate_seg(..., sweep=True)), then one row per class
    with the subject `pooled` from the summed histograms: THRESHOLD_COLUMNS.  dsc is the Dice at the default decision
    (metrics.csv's), best_thr_logit the edge of the best Dice as %.9g (the fp32 value reads back exactly),
    best_thr_prob its sigmoid in fp64."""
    per, pooled, _ = sweep_results(results)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(THRESHOLD_COLUMNS)
        for name, summ in per + [("pooled", pooled)]:
            for c, q in enumerate(summ):
                wr.writerow([name, c, "%.9g" % q["auc"], "%.7g" % float(q["dsc_default"]), "%.9g" % q["best_thr"],
                             "%.9g" % logit_prob(q["best_thr"])] +
                            ["%.7g" % float(q[k]) for k in ("dsc_best", "sens_best", "spec_best")] + [q["pos"], q["neg"]])


def write_threshold_curve_csv(path: str, results) -> None:
    """The pooled curve of the "sweep" entries, one row per class and k = 1 .. 4095: THRESHOLD_CURVE_COLUMNS, the counts
    of the decision "score >= edge k" summed over the subjects and their dsc, sens and spec (metrics_from_counts)."""
    _, pooled, edges = sweep_results(results)
    e = [float(v) for v in torch.as_tensor(edges).tolist()]
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(THRESHOLD_CURVE_COLUMNS)
        for c, q in enumerate(pooled):
            m = metrics_from_counts(q["counts"])
            for k in range(1, SWEEP_BINS):
                wr.writerow([c, k, "%.9g" % e[k], "%.9g" % logit_prob(e[k])] + [int(v) for v in q["counts"][k]] +
                            ["%.7g" % float(m[j][k]) for j in ("dsc", "sens", "spec")])


def write_metrics_post_csv(path: str, results) -> None:
    """One row per subject and class from the "post" entries (validate_seg(..., post=...)): subject, class, dsc, sens,
    spec, acc, tp, fp, fn, tn of the cleaned map, then changed_<k>, the voxels rule k relabelled in the subject's map
    (the same in every row of a subject)."""
    rows = [r for r in results if "post" in r]
    nrules = max((len(r["post"]["changed"]) for r in rows), default=0)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + METRICS + ("tp", "fp", "fn", "tn") +
                    tuple(f"changed_{k}" for k in range(nrules)))
        for r in rows:
            q = r["post"]
            for c in range(q["counts"].shape[0]):
                wr.writerow([r["name"], c] + ["%.7g" % float(q[m][c]) for m in METRICS] +
                            [int(v) for v in q["counts"][c]] + [int(v) for v in q["changed"]])


def write_agreement_csv(path: str, results) -> None:
    """One row per subject and class from the "vs_fp" entries (validate_seg(..., fp_model=...)): subject, class, dsc,
    sens, spec, acc, both, q_only, fp_only, neither, flip_frac_class = (q_only + fp_only) / voxels, logit_rel_mse,
    logit_max, prob_mae, and when the entries carry "lesions" / "surface" (against the FP decisions) the columns of
    write_metrics_csv after them, under its names and its unit rule; a file never mixes voxel units and mm."""
    vs = [(r["name"], r["vs_fp"]) for r in results if "vs_fp" in r]
    cols, values = _lesion_surface_columns([v for _, v in vs], "write_agreement_csv")
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + METRICS + AGREEMENT_COUNTS + ("flip_frac_class",) + AGREEMENT_DRIFT + cols)
        for name, v in vs:
            for c in range(v["counts"].shape[0]):
                row = [int(n) for n in v["counts"][c]]
                wr.writerow([name, c] + ["%.7g" % float(v[m][c]) for m in METRICS] + row +
                            ["%.7g" % ((row[1] + row[2]) / sum(row))] +
                            ["%.7g" % float(v[k][c]) for k in AGREEMENT_DRIFT] + values(v, c))


def write_lesions_csv(path: str, results) -> None:
    """One row per lesion of results that carry "lesion_table" (validate_seg(..., lesion_table=True)): subject, class,
    kind (label | pred), lesion (1-based, in raster order of the first voxel: scipy.ndimage.label's number), d, h, w of
    the first voxel, size in voxels, overlap; per subject and class the label lesions first.  When the results carry a
    "spacing" a last column vol_mm3 = size x voxel volume; a file never mixes rows with and without it.  When they carry
    "lesion_match" (validate_seg(..., lesion_match=True)) three more columns after all others: match (the 1-based number
    of the lesion of the other kind matched one to one at IoU > 0.5, or 0), best_iou (the largest IoU with any lesion of
    the other kind, or 0) and partners (how many of them it shares voxels with); again a file never mixes the two."""
    res = [r for r in results if "lesion_table" in r]
    mm = {"spacing" in r for r in res}
    if len(mm) > 1:
        raise RuntimeError("write_lesions_csv: cases with and without a spacing in one file")
    mm = mm == {True}
    lm = {"lesion_match" in r for r in res}
    if len(lm) > 1:
        raise RuntimeError("write_lesions_csv: cases with and without a lesion matching in one file")
    lm = lm == {True}
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class", "kind", "lesion") + LESION_TABLE_COLUMNS + (("vol_mm3",) if mm else ()) +
                    (("match", "best_iou", "partners") if lm else ()))
        for r in res:
            vox = float(np.prod([float(v) for v in r["spacing"]])) if mm else None
            for c, pair in enumerate(r["lesion_table"]):
                for kind, rows in zip(("label", "pred"), pair):
                    side = r["lesion_match"][c][kind] if lm else None
                    for k, row in enumerate(np.asarray(rows, dtype=np.int64).reshape(-1, 5)):
                        wr.writerow([r["name"], c, kind, k + 1] + [int(v) for v in row] +
                                    (["%.7g" % (int(row[3]) * vox)] if mm else []) +
                                    ([int(side["match"][k]), "%.7g" % float(side["best_iou"][k]),
                                      int(side["partners"][k])] if lm else []))


# ---- what the ptq mission prints of a validation (entrance._ValidationTester) ------------------------------------------
def metric_lines(folder: str, res, seconds: float, is_cc: bool, is_surf: bool) -> list:
    """The per-class means of a labelled validation, with the lesion totals of --is_cc and the mean surface distances
    of --surf_dist."""
    means = metric_means(res)
    lines = [f'[entrance] {folder}: {len(res)} val cases in {seconds:.2f}s, per-class means:']
    tot = lesion_totals(res) if is_cc else None
    surf = surface_means(res) if is_surf else None
    for c in range(len(means['dsc'])):
        line = f'  class {c}: ' + ', '.join(f'{m} = {float(means[m][c]):.4f}' for m in METRICS)
        if is_cc:
            line += ', ' + ', '.join(f'{k} = {int(tot[c][j])}' for j, k in enumerate(LESION_COLUMNS))
        if is_surf:
            mm = ' mm' if res[0].get('surface_unit') == 'mm' else ''
            line += ', ' + ', '.join(f'{k} = {float(surf[c][j]):.3f}{mm}' for j, k in enumerate(SURFACE_COLUMNS))
        lines.append(line)
    return lines


def lesion_size_lines(folder: str, res) -> list:
    """--lesion_table: the detected label lesions per class and size bin."""
    bins = lesion_size_summary(res)
    names = [f'{lo}-{hi}' if hi is not None else f'>= {lo}' for lo, hi in LESION_SIZE_BINS]
    return [f'[entrance] {folder}: label lesions detected / all, by size in voxels:'] + \
        [f'  class {c}: ' + ', '.join(f'{n}: {int(k[1])} / {int(k[0])}' for n, k in zip(names, bins[c]))
         for c in range(bins.shape[0])]


def lesion_match_lines(folder: str, res) -> list:
    """--lesion_match: lesion_match.match_summary per class."""
    from .lesion_match import match_summary
    return [f'[entrance] {folder}: lesions matched one to one at IoU > 0.5, per class the mean f1_l, pq and lw_dsc '
            f'and the pooled tp_l / fp_l / fn_l:'] + \
        [f'  class {c}: f1_l = {m["f1_l"]:.4f}, pq = {m["pq"]:.4f}, lw_dsc = {m["lw_dsc"]:.4f}, '
         f'tp_l / fp_l / fn_l = {m["tp_l"]} / {m["fp_l"]} / {m["fn_l"]}' for c, m in enumerate(match_summary(res))]


def post_lines(folder: str, res, rules_said: str, nrules: int) -> list:
    """--post: the voxels each of the `nrules` rules relabelled and the mean Dice before and after; `rules_said` is
    config.post_text of the rules."""
    means, after = metric_means(res), post_means(res)
    changed = [sum(r['post']['changed'][k] for r in res) for k in range(nrules)]
    return [f'[entrance] {folder}: --post {rules_said}: '
            f'{" ".join(str(v) for v in changed)} voxels relabelled, per-class mean dsc before -> after:'] + \
        [f'  class {c}: {float(means["dsc"][c]):.4f} -> {float(after["dsc"][c]):.4f}' for c in range(len(means['dsc']))]


def sweep_means(res) -> tuple:
    """(mean AUC per class, pooled summary) of the results that carry a sweep: one network's entry of sweep_lines."""
    per, pooled, _ = sweep_results(res)
    return [sum(s[c]['auc'] for _, s in per) / len(per) for c in range(len(pooled))], pooled


def sweep_lines(folder: str, swept: dict, sigmoid: bool) -> list:
    """--thr_sweep: per class the mean AUC, the pooled best threshold and the pooled Dice at the default threshold and at
    the best, every network of `swept` (folder -> sweep_means) side by side; `folder` is the one just swept."""
    def said(name, c):
        auc, pool = swept[name]
        q = pool[c]
        at = f'{logit_prob(q["best_thr"]):.4f} (logit {q["best_thr"]:.9g})' if sigmoid else f'margin {q["best_thr"]:.9g}'
        return (f'{name.upper()}: AUC {auc[c]:.4f}, Dice {float(q["dsc_default"]):.4f} at '
                f'{"0.5" if sigmoid else "argmax"}, {float(q["dsc_best"]):.4f} at {at}')
    return [f'[entrance] {folder}: --thr_sweep, per class the mean AUC and the pooled Dice at the default and at the '
            f'best threshold:'] + \
        [f'  class {c}: ' + '; '.join(said(name, c) for name in swept) for c in range(len(swept[folder][1]))]


def agreement_lines(folder: str, res) -> list:
    """--vs_fp: the share of voxels decided differently and the per-class means of the agreement."""
    m = agreement_means(res)
    return [f'[entrance] {folder} against the FP network: {100 * m["flip_frac"]:.4f} % of the voxels decided '
            f'differently, per-class means:'] + \
        [f'  class {c}: dsc = {float(m["dsc"][c]):.4f}, logit_rel_mse = {float(m["logit_rel_mse"][c]):.4g}, '
         f'prob_mae = {float(m["prob_mae"][c]):.4g}' for c in range(len(m['dsc']))]
