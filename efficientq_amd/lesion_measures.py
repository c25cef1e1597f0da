"""The host side of ``--lesion_measures`` (score, predict): the slice axis of a map, the rows of ``lesions.csv`` from the
records of ops_measure.label_lesion_measures, and the detection table by diameter of ``lesion_detect.csv``.  Host values
only; the device call is ops_measure's."""
from __future__ import annotations

import csv
import math
from typing import List, Sequence

import numpy as np

from . import prep
from ._lib import LESION_MEASURE_WORDS as MEASURE_WORDS
from .prep import PrepError

LESIONS_CSV, DETECT_CSV = "lesions.csv", "lesion_detect.csv"
PLANE_AXES = ("d", "h", "w")          # array axes 0, 1, 2
LESION_COLUMNS = ("subject", "class", "labels", "kind", "lesion", "d", "h", "w", "size", "overlap", "vol_ml", "cd", "ch",
                  "cw", "x_mm", "y_mm", "z_mm", "box_lo", "box_hi", "diam_mm", "diam_from", "diam_to", "plane",
                  "plane_diam_mm", "plane_from", "plane_to")
DETECT_COLUMNS = ("class", "labels", "bin", "labelled", "detected", "invented")
# the bins of lesion_detect.csv over diam_mm: name, from (inclusive), to (exclusive)
DIAMETER_BINS = (("<5", 0.0, 5.0), ("5-10", 5.0, 10.0), ("10-20", 10.0, 20.0), (">=20", 20.0, math.inf))


def slice_axis(plane: str, affine, subject: str) -> int:
    """The array axis the slices of `plane` are stacked along: d, h, w name it; axial is the axis that
    prep.scan_orientation of `affine` puts nearest to world z.  An affine that function refuses is refused naming the
    subject."""
    if plane in PLANE_AXES:
        return PLANE_AXES.index(plane)
    try:
        world, _ = prep.scan_orientation(affine)
    except PrepError as e:
        raise PrepError(f"subject {subject}: --measure_plane axial: {e}: name the array axis the slices are stacked along "
                        f"with --measure_plane d|h|w")
    return world.index(2)


def diameter_mm(a: Sequence[int], b: Sequence[int], spacing) -> float:
    """sqrt(sum((spacing_a (b_a - a_a)) ** 2)) in fp64, between the centres of two voxels."""
    return math.sqrt(sum((float(s) * (int(q) - int(p))) ** 2 for p, q, s in zip(a, b, spacing)))


def lesion_rows(subject: str, classes, with_truth: bool, rows, meas, shape, spacing, affine, axis: int) -> List[dict]:
    """The rows of lesions.csv of one subject, unformatted: per class the label lesions (with_truth: plane C + c) first,
    then the predicted ones (plane c), each in raster order of the first voxel.  `rows` and `meas`: the lists of
    ops_measure.label_lesion_measures; `spacing` and `affine`: the header's; `axis`: the slice axis of the call."""
    C = len(classes)
    ml = float(np.prod([float(v) for v in spacing])) / 1000.0
    A = np.asarray(affine, dtype=np.float64)
    out = []

    def at(v):
        return tuple(int(x) for x in np.unravel_index(int(v), shape))
    for c, labels in enumerate(classes):
        for kind, q in (("label", C + c), ("pred", c)) if with_truth else (("pred", c),):
            table, records = np.asarray(rows[q], dtype=np.int64).reshape(-1, 3), np.asarray(meas[q], dtype=np.int64)
            for k, ((first, size, overlap), m) in enumerate(zip(table, records.reshape(len(table), MEASURE_WORDS))):
                centre = [int(s) / int(size) for s in m[0:3]]
                world = [sum(A[i, a] * centre[a] for a in range(3)) + A[i, 3] for i in range(3)]
                ends = [at(m[j]) for j in (9, 10, 11, 12)]
                d, h, w = at(first)
                out.append({"subject": subject, "class": c, "labels": prep._fmt(labels), "kind": kind, "lesion": k + 1,
                            "d": d, "h": h, "w": w, "size": int(size), "overlap": int(overlap), "vol_ml": int(size) * ml,
                            "cd": centre[0], "ch": centre[1], "cw": centre[2], "x_mm": float(world[0]),
                            "y_mm": float(world[1]), "z_mm": float(world[2]), "box_lo": prep._fmt(m[3:6]),
                            "box_hi": prep._fmt(m[6:9]), "diam_mm": diameter_mm(ends[0], ends[1], spacing),
                            "diam_from": prep._fmt(ends[0]), "diam_to": prep._fmt(ends[1]), "plane": PLANE_AXES[axis],
                            "plane_diam_mm": diameter_mm(ends[2], ends[3], spacing), "plane_from": prep._fmt(ends[2]),
                            "plane_to": prep._fmt(ends[3])})
    return out


def detect_rows(classes, lesions: List[dict]) -> List[dict]:
    """The rows of lesion_detect.csv: per class and bin of diam_mm the label lesions, those of them with overlap > 0, and
    the predicted lesions with overlap 0."""
    out = []
    for c, labels in enumerate(classes):
        mine = [r for r in lesions if r["class"] == c]
        for name, lo, hi in DIAMETER_BINS:
            inside = [r for r in mine if lo <= r["diam_mm"] < hi]
            label = [r for r in inside if r["kind"] == "label"]
            out.append({"class": c, "labels": prep._fmt(labels), "bin": name, "labelled": len(label),
                        "detected": sum(1 for r in label if r["overlap"] > 0),
                        "invented": sum(1 for r in inside if r["kind"] == "pred" and r["overlap"] == 0)})
    return out


def detect_said(rows: List[dict], c: int) -> str:
    """The numbers of class c of detect_rows in one line: `<5 mm 2/3 +1` = detected / labelled, invented."""
    return ", ".join(f"{r['bin']} mm {r['detected']}/{r['labelled']} +{r['invented']}" for r in rows if r["class"] == c)


def write_csv(path: str, header, rows: List[dict]) -> None:
    def dump(p):
        with open(p, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(header)
            w.writerows(["%.7g" % r[k] if isinstance(r[k], float) else r[k] for k in header] for r in rows)
    prep._replace(path, dump)
