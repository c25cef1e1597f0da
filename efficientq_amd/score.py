"""The ``score`` mission: finished label maps against the labels of the list, on the scan's own grid.

    python -m efficientq_amd.entrance score --task lits --src_list cases.csv --pred_dir seg/ --out_dir score/ \
        [--score_class 1,2 --score_class 2] [--score_tol 1,3]

``--src_list`` is the CSV of ``prep`` and ``predict`` (prep.read_src_list).  The truth of a subject is its ``seg`` cell,
its map is ``<pred_dir>/<subject>.nii.gz`` (or ``.nii``) - what ``predict`` wrote, after ``--post`` and everything else,
or the map of any other tool.  A subject with an empty ``seg`` cell is skipped and named in one line.  A list without a
``seg`` column, a list with no labelled subject and a missing map are refused before the device or ``--out_dir`` is
touched; so is a subject whose map and label do not lie on one grid (prep.check_same_grid on the two headers) or whose
2 C planes exceed the limits of the device calls.  The values of both images must be integers of 0 to 255 (``scl_slope``
applied); the first value that is not stops the run, named with its subject and file.

Class c of a map is "the voxel's value is one of the labels of class c" (``--score_class LABELS``, repeatable; per task
config.SCORE_CLASSES), so classes may nest.  Per subject three device calls on the two uint8 maps: ``ops.label_tallies``
(TP, FP, FN, TN), ``ops_score.label_lesions`` (the 26-neighbourhood lesion counts of ``--is_cc``) and
``ops_score.label_surface_mm`` (the 6-neighbour surfaces of ``--surf_dist`` in the millimetres of the map's header, and
the surface voxels within every ``--score_tol`` of the other surface).

``<out_dir>/scores.csv``: one row per subject and class - ``subject, class, labels, dsc, sens, spec, acc, tp, fp, fn, tn,
pred_ml, label_ml, totall, predl, fnl, fpl, hd_mm, hd95_mm, assd_mm`` and one ``nsd_<T>mm`` per tolerance.  The ratios
are metrics.metrics_from_counts', the volumes voxels x the product of the spacing / 1000, the distances
metrics.surface_metrics_mm's, and the normalised surface Dice (nsd) is (within_P + within_L) / (nP + nL): the share of
the surface voxels of both masks that lie within T mm of the other surface; 1 when both surfaces are empty, 0 when
exactly one is.  ``<out_dir>/summary.csv``: one row per class - the cases, the means of ``dsc``, ``hd95_mm``, ``assd_mm``
and every ``nsd_*``, the summed lesion counts, ``lesion_sens = 1 - fnl / totall`` and ``lesion_prec = 1 - fpl / predl``
(each 1 when its denominator is 0).  Floats are printed as metrics.csv prints them (``%.7g``).

``--lesion_measures`` (``--measure_plane axial|d|h|w``): one more device call per subject on the same two maps,
``ops_measure.label_lesion_measures``, and two more files, lesion_measures.py's: ``<out_dir>/lesions.csv``, one row per
connected component of every class (place, size, overlap, volume in ml, centroid in voxels and in scanner coordinates, box,
the longest diameter in mm in 3-D and inside one slice with their end points), and ``<out_dir>/lesion_detect.csv``, the
label lesions, the detected ones and the invented ones per class and bin of the diameter.  The slice axis of every
subject is resolved from its header before the device is touched; the other two files are what they are without it.
"""
from __future__ import annotations

import csv
import os
import os.path as P
from functools import partial
from types import SimpleNamespace
from typing import List

import numpy as np
import torch

from . import _lib
from . import config as Cf
from . import data as D
from . import lesion_measures as LM
from . import metrics as M
from . import nifti
from . import prep
from .prep import PrepError

SCORES_CSV, SUMMARY_CSV = "scores.csv", "summary.csv"
SCORE_COLUMNS = ("subject", "class", "labels") + M.METRICS + ("tp", "fp", "fn", "tn", "pred_ml", "label_ml") + \
    M.LESION_COLUMNS + M.SURFACE_COLUMNS_MM
SUMMARY_MEANS = ("dsc", "hd95_mm", "assd_mm")
MAP_SUFFIXES = (".nii.gz", ".nii")


def nsd_column(tol: float) -> str:
    return "nsd_%gmm" % tol


def nsd(within_p: int, within_l: int, n_p: int, n_l: int) -> float:
    """The normalised surface Dice from the surface voxels of each mask within the tolerance of the other surface and
    the sizes of the two surfaces: 1 when both are empty, 0 when exactly one is."""
    if n_p == 0 and n_l == 0:
        return 1.0
    if n_p == 0 or n_l == 0:
        return 0.0
    return (int(within_p) + int(within_l)) / (int(n_p) + int(n_l))


def lesion_rates(totall: int, predl: int, fnl: int, fpl: int):
    """(lesion_sens, lesion_prec) = (1 - fnl / totall, 1 - fpl / predl), each 1 when its denominator is 0."""
    return (1.0 - fnl / totall if totall else 1.0, 1.0 - fpl / predl if predl else 1.0)


def _has_seg_column(path: str) -> bool:
    with open(path, "r", newline="") as f:
        for r in csv.reader(f):
            if any(c.strip() for c in r):
                return D.LABEL_MODALITY in [c.strip() for c in r]
    return False


def _resolve(args) -> SimpleNamespace:
    """Everything `args`, the list and the headers decide, refused by name before anything touches the device or out_dir;
    returns the mission's job: host values only."""
    classes, tols = Cf.score_switches(args, "score")
    measures = Cf.measure_switches(args, "score")
    task = (getattr(args, "task", None) or "").lower()
    if task not in D.MODALITIES:
        raise PrepError(f"score: --task {getattr(args, 'task', None)!r}, one of {', '.join(D.MODALITIES)}")
    for switch in ("src_list", "pred_dir", "out_dir"):
        if not getattr(args, switch, None):
            raise PrepError("score: needs --src_list, --pred_dir and --out_dir")
    entries = prep.read_src_list(args.src_list, task)
    if not _has_seg_column(args.src_list):
        raise PrepError(f"--src_list {args.src_list}: no {D.LABEL_MODALITY} column: the score mission scores maps against "
                        f"the labels it names")
    skipped = [e["subject"] for e in entries if not e["seg"]]
    cases = []
    for e in entries:
        if not e["seg"]:
            continue
        found = [P.join(args.pred_dir, e["subject"] + s) for s in MAP_SUFFIXES]
        found = [p for p in found if P.isfile(p)]
        if not found:
            raise PrepError(f"--pred_dir {args.pred_dir}: subject {e['subject']}: no map {e['subject']}{MAP_SUFFIXES[0]} "
                            f"(or {MAP_SUFFIXES[1]})")
        cases.append(SimpleNamespace(subject=e["subject"], pred=found[0], seg=e["seg"]))
    if not cases:
        raise PrepError(f"--src_list {args.src_list}: no subject has a {D.LABEL_MODALITY} cell: nothing to score against")
    C = len(classes)
    for c in cases:
        try:
            gp, gl = nifti.read_geometry(c.pred), nifti.read_geometry(c.seg)
        except (ValueError, OSError) as e:
            raise PrepError(f"subject {c.subject}: {e}")
        try:
            prep.check_same_grid(c.subject, gp, gl, f"the label {c.seg}")
        except PrepError as e:
            raise PrepError(f"{e} (the first modality is here the map {c.pred}: the score mission needs both on one grid)")
        shape = tuple(int(n) for n in gp["shape"][:3])
        if len(gp["shape"]) > 3 and any(int(n) != 1 for n in gp["shape"][3:]):
            raise PrepError(f"subject {c.subject}: {c.pred}: shape {tuple(gp['shape'])}: a label map has three axes")
        if 2 * C * int(np.prod(shape)) >= 2 ** 31 or max(shape) > _lib.EDT_MM_MAX_EXTENT:
            raise PrepError(f"subject {c.subject}: {2 * C} masks of {prep._fmt(shape)} voxels are outside the limits of "
                            f"the device calls (2^31 - 1 voxels in all, every extent at most {_lib.EDT_MM_MAX_EXTENT})")
        c.shape, c.spacing = shape, tuple(float(v) for v in gp["spacing"])
        if not all(np.isfinite(v) and v > 0 for v in c.spacing):
            raise PrepError(f"subject {c.subject}: {c.pred}: spacing {c.spacing}: needs three finite positive numbers")
        if measures:
            c.affine = np.asarray(gp["affine"], dtype=np.float64)
            c.slice_axis = LM.slice_axis(measures[1], c.affine, c.subject)
    return SimpleNamespace(task=task, classes=classes, tols=tols, lut=Cf.score_class_lut(classes), cases=cases,
                           skipped=skipped, measures=bool(measures))


def read_labels(subject: str, path: str) -> np.ndarray:
    """The uint8 label map of a NIfTI image whose every value (scl_slope applied) is an integer of 0 to 255; the first
    value that is not is refused naming subject, file and value."""
    try:
        a, _ = nifti.read_image(path)
    except (ValueError, OSError) as e:
        raise PrepError(f"subject {subject}: {e}")
    with np.errstate(invalid="ignore"):
        bad = ~((a >= 0) & (a <= 255) & (a == np.floor(a)))
    if bad.any():
        at = np.unravel_index(int(np.argmax(bad)), a.shape)
        raise PrepError(f"subject {subject}: {path}: value {float(a[at]):g} at voxel {prep._fmt(at)} is no label: every "
                        f"value of a label map is an integer of 0 to 255")
    return np.ascontiguousarray(a.astype(np.uint8))


def device_calls(ops) -> SimpleNamespace:
    """The three device calls of a subject over `ops` (a HipOps), and the fourth of --lesion_measures."""
    from . import ops_measure as OM
    from . import ops_score as OS
    return SimpleNamespace(tallies=ops.label_tallies, lesions=partial(OS.label_lesions, ops),
                           surface=partial(OS.label_surface_mm, ops), measures=partial(OM.label_lesion_measures, ops))


def score_case(calls, device, job, case, measured=None) -> List[dict]:
    """The rows of scores.csv of one subject, unformatted: one dict per class.  `measured` (a list, with
    --lesion_measures): the subject's rows of lesions.csv are added to it, from one more call on the same two maps."""
    pred = torch.from_numpy(read_labels(case.subject, case.pred)).to(device)
    truth = torch.from_numpy(read_labels(case.subject, case.seg)).to(device)
    C = len(job.classes)
    counts = calls.tallies(pred, truth, job.lut, C).cpu()
    lesions = calls.lesions(pred, truth, job.lut, C).cpu()
    n, sq, sums, within = (t.cpu() for t in calls.surface(pred, truth, job.lut, C, case.spacing, job.tols))
    if measured is not None:
        try:
            _, _, table, meas = calls.measures(pred, truth, job.lut, C, case.spacing, case.slice_axis)
        except _lib.EffqError as e:
            raise PrepError(f"subject {case.subject}: --lesion_measures: {e}")
        measured += LM.lesion_rows(case.subject, job.classes, True, table, meas, case.shape, case.spacing, case.affine,
                                  case.slice_axis)
    ratios = M.metrics_from_counts(counts)
    surface = M.surface_metrics_mm(n, sq, sums, case.shape, case.spacing)
    ml = float(np.prod(case.spacing)) / 1000.0
    rows = []
    for c, labels in enumerate(job.classes):
        tp, fp, fn, tn = (int(v) for v in counts[c])
        row = {"subject": case.subject, "class": c, "labels": prep._fmt(labels), "tp": tp, "fp": fp, "fn": fn, "tn": tn,
               "pred_ml": (tp + fp) * ml, "label_ml": (tp + fn) * ml}
        row.update({m: float(ratios[m][c]) for m in M.METRICS})
        row.update({k: int(v) for k, v in zip(M.LESION_COLUMNS, lesions[c])})
        row.update({k: float(v) for k, v in zip(M.SURFACE_COLUMNS_MM, surface[c])})
        for k, tol in enumerate(job.tols):
            row[nsd_column(tol)] = nsd(int(within[c, 0, k]), int(within[c, 1, k]), int(n[c, 0]), int(n[c, 1]))
        rows.append(row)
    return rows


def summarise(job, rows: List[dict]) -> List[dict]:
    """The rows of summary.csv, unformatted: one dict per class over the rows of scores.csv."""
    out = []
    for c, labels in enumerate(job.classes):
        mine = [r for r in rows if r["class"] == c]
        row = {"class": c, "labels": prep._fmt(labels), "cases": len(mine)}
        for k in SUMMARY_MEANS + tuple(nsd_column(t) for t in job.tols):
            row[k] = sum(r[k] for r in mine) / len(mine)
        row.update({k: sum(r[k] for r in mine) for k in M.LESION_COLUMNS})
        row["lesion_sens"], row["lesion_prec"] = lesion_rates(*(row[k] for k in M.LESION_COLUMNS))
        out.append(row)
    return out


def summary_columns(tols) -> tuple:
    return ("class", "labels", "cases") + SUMMARY_MEANS + tuple(nsd_column(t) for t in tols) + M.LESION_COLUMNS + \
        ("lesion_sens", "lesion_prec")


def _cell(v):
    return "%.7g" % v if isinstance(v, float) else v


def _write_csv(path: str, header, rows: List[dict]) -> None:
    def dump(p):
        with open(p, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(header)
            w.writerows([_cell(r[k]) for k in header] for r in rows)
    prep._replace(path, dump)


def _means_said(job, row: dict) -> str:
    return " ".join(f"{k} {row[k]:.4g}" for k in SUMMARY_MEANS + tuple(nsd_column(t) for t in job.tols))


def run(args, ops=None, calls=None) -> List[dict]:
    """The `score` mission of `args` (config.build_parser); returns the rows of scores.csv, unformatted.  `ops`: the
    HipOps whose device holds the maps (hip_ops.get_ops(args.device) by default); `calls`: the three device calls
    (device_calls(ops) by default)."""
    job = _resolve(args)
    if calls is None:
        if ops is None:
            from .hip_ops import get_ops
            ops = get_ops(torch.device("cuda", int(getattr(args, "device", 0) or 0)))
        calls = device_calls(ops)
    device = ops.device if ops is not None else torch.device("cpu")
    os.makedirs(args.out_dir, exist_ok=True)
    if job.skipped:
        print(f"[score] {len(job.skipped)} subjects without a {D.LABEL_MODALITY} cell are skipped: {' '.join(job.skipped)}")
    rows, lesions = [], [] if job.measures else None
    for case in job.cases:
        mine = score_case(calls, device, job, case, lesions)
        rows += mine
        print(f"[score] {case.subject}: {prep._fmt(case.shape)} at {prep._fmt(case.spacing)} mm: " +
              "; ".join(f"class {r['class']} {_means_said(job, r)} lesions {r['totall']}/{r['predl']} missed "
                        f"{r['fnl']} invented {r['fpl']}" for r in mine))
    summary = summarise(job, rows)
    _write_csv(P.join(args.out_dir, SCORES_CSV), SCORE_COLUMNS + tuple(nsd_column(t) for t in job.tols), rows)
    _write_csv(P.join(args.out_dir, SUMMARY_CSV), summary_columns(job.tols), summary)
    for r in summary:
        print(f"[score] class {r['class']} (labels {r['labels']}), {r['cases']} cases: mean {_means_said(job, r)}, "
              f"lesion_sens {r['lesion_sens']:.4g} lesion_prec {r['lesion_prec']:.4g}")
    if job.measures:
        detect = LM.detect_rows(job.classes, lesions)
        LM.write_csv(P.join(args.out_dir, LM.LESIONS_CSV), LM.LESION_COLUMNS, lesions)
        LM.write_csv(P.join(args.out_dir, LM.DETECT_CSV), LM.DETECT_COLUMNS, detect)
        for c, labels in enumerate(job.classes):
            print(f"[score] class {c} (labels {prep._fmt(labels)}), detected / labelled +invented by diameter: "
                  f"{LM.detect_said(detect, c)}")
        print(f"[score] {len(lesions)} lesions measured: {P.join(args.out_dir, LM.LESIONS_CSV)}, "
              f"{P.join(args.out_dir, LM.DETECT_CSV)}")
    print(f"[score] {len(job.cases)} subjects scored: {P.join(args.out_dir, SCORES_CSV)}, "
          f"{P.join(args.out_dir, SUMMARY_CSV)}")
    return rows
