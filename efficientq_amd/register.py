"""Rigid registration of one modality onto the reference by mutual information (--prep_register rigid of the ``prep`` and
``predict`` missions).  The one definition of the rule; host code in fp64, the device evaluates the
objective (ops_register.prep_bins, ops_register.prep_joint_hist; csrc/prep_register.hip).

Transform   theta = (tx, ty, tz in mm, rx, ry, rz in radians): the rotation Rz Ry Rx about the world centre of the
            reference grid, then the translation.  M(theta) = inv(A_src) T(theta) A_ref (3 x 4, fp64) maps a voxel index of
            the reference grid to voxel coordinates of the moving scan, as prep.align_matrix does; M(0) is
            prep.align_matrix bit for bit (the product with T is skipped), so "before" is the alignment by the headers.
Objective   the normalised mutual information (H_f + H_m) / H_fm of one BINS x BINS joint histogram (nmi).  A candidate
            whose histogram holds fewer than half the samples of theta = 0 is rejected: the search cannot walk the scan
            out of the field of view.
Bins        per volume lo, hi = its 0.5 and 99.5 percentile over its mask (the radix select of --prep_window pLO,pHI),
            scale = float32(BINS / (hi - lo)); hi <= lo stops the run, naming the subject and the modality.
Search      a deterministic pattern search over the levels of sample stride 4, 2, 1; a level that would leave fewer than
            MIN_SAMPLES samples along an axis is dropped (stride 1 always runs).  At stride s > 1 both volumes are smoothed
            with prep_smooth, sigma = prep.antialias_sigma of the factor s (the moving volume: s times the finest reference
            spacing over its own spacing, per axis).  A launch evaluates 13 candidates: theta, and theta +- step in each of
            the six parameters (index 1 + 2 p for +, 2 + 2 p for -).  The best candidate, ties to the lowest index, is
            moved to when it is strictly better than theta; otherwise the step is halved.  A level starts with a step of two
            sample strides of the finest reference spacing - for the rotations the angle that moves the farthest grid
            corner by that much - and ends when the step is below 1/8 of its sample stride, or after MAX_LAUNCHES launches
            (recorded as converged 0; no error).  Every level begins with one launch at theta = 0 for the sample count.
Out of scope: affine and deformable transforms, an initialisation by centre of mass (the search is local and starts from
the headers), the label, registration between subjects, partial-volume or Parzen histograms, other similarity measures.
"""
from __future__ import annotations

import math
from collections import namedtuple
from functools import partial
from typing import Sequence

import numpy as np

from . import ops_register
from . import prep

BINS = ops_register.BINS
STRIDES = (4, 2, 1)
MIN_SAMPLES = 16
MAX_LAUNCHES = 200
PERCENTILES = (0.5, 99.5)
REGISTER_KINDS = ("rigid",)

# theta, M(theta), the NMI at theta = 0 and at theta on the full grid, the launches, and whether no level hit the cap.
# `matrix` and `nmi_after` belong to theta as the search left it; the missions apply M(params_theta(params_text(theta))),
# whose rotations went through degrees and back and may differ from theta's in the last bit.
Registered = namedtuple("Registered", "theta matrix nmi_before nmi_after evals converged")


def register_switch(args, align):
    """--prep_register of `args` (or the YAML key): 'rigid', None when the switch is absent; any other value is refused by
    name, and so is the switch without --prep_align, which names the reference."""
    kind = getattr(args, "prep_register", None)
    if kind is None:
        return None
    if not isinstance(kind, str) or kind.strip().lower() not in REGISTER_KINDS:
        raise prep.PrepError(f"--prep_register {kind!r}: rigid")
    if align is None:
        raise prep.PrepError("--prep_register rigid registers every other modality onto the reference: it needs "
                             "--prep_align MODALITY to name the reference")
    return kind.strip().lower()


def rigid_transform(theta: Sequence[float], centre) -> np.ndarray:
    """T(theta), 4 x 4 in world coordinates: x -> Rz Ry Rx (x - centre) + centre + t."""
    tx, ty, tz, rx, ry, rz = (float(v) for v in theta)
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    r = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) \
        @ np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    c = np.asarray(centre, dtype=np.float64)
    t = np.eye(4)
    t[:3, :3] = r
    t[:3, 3] = (c - r @ c) + np.array([tx, ty, tz])
    return t


def grid_centre(a_ref, ref_shape) -> np.ndarray:
    """The world position of the centre of the reference grid, the voxel coordinate (n - 1) / 2."""
    a = np.asarray(a_ref, dtype=np.float64)
    return a[:3, :3] @ ((np.asarray(ref_shape, dtype=np.float64) - 1.0) / 2.0) + a[:3, 3]


def rigid_matrix(subject: str, name: str, a_src, a_ref, ref_shape, theta) -> np.ndarray:
    """M(theta) = inv(A_src) T(theta) A_ref as 3 x 4 fp64; theta = 0 is prep.align_matrix itself."""
    a_ref = np.asarray(a_ref, dtype=np.float64)
    if not any(float(v) != 0.0 for v in theta):
        return prep.align_matrix(subject, name, a_src, a_ref)
    return prep.align_matrix(subject, name, a_src, rigid_transform(theta, grid_centre(a_ref, ref_shape)) @ a_ref)


def nmi(hist) -> float:
    """(H_f + H_m) / H_fm of one joint histogram, fp64, natural log, empty bins skipped, every sum in raster order.  A
    histogram without a sample, or with all samples in one cell (H_fm = 0), has no information: 0."""
    h = np.asarray(hist, dtype=np.float64)
    total = float(h.sum())

    def entropy(counts) -> float:
        e = 0.0
        for v in counts:
            if v > 0.0:
                p = v / total
                e -= p * math.log(p)
        return e
    if total <= 0.0:
        return 0.0
    rows, cols = h.sum(1).tolist(), h.sum(0).tolist()           # sums of integers: exact in fp64 in any order
    joint = entropy(h.reshape(-1).tolist())
    return (entropy(rows) + entropy(cols)) / joint if joint > 0.0 else 0.0


def candidates(theta, step_mm: float, step_rad: float):
    """The 13 candidates of one launch: theta, then theta + step and theta - step in each parameter in turn."""
    out = [tuple(theta)]
    for p in range(6):
        for sign in (1.0, -1.0):
            c = list(theta)
            c[p] = c[p] + sign * (step_mm if p < 3 else step_rad)
            out.append(tuple(c))
    return out


def params_text(theta) -> str:
    """`tx ty tz rx ry rz` as prep.csv and predict.csv record them: millimetres and degrees, repr(float)."""
    return " ".join(repr(float(v)) for v in list(theta[:3]) + [math.degrees(r) for r in theta[3:]])


def params_theta(text: str) -> tuple:
    """theta from params_text's record.  The missions resample with M(params_theta(params_text(theta))): the matrix that
    was applied can be formed again from the file, bit for bit."""
    v = [float(s) for s in text.split()]
    return tuple(v[:3] + [math.radians(d) for d in v[3:]])


def rotation_degrees(theta) -> float:
    """The angle of the rotation Rz Ry Rx as one turn about its axis."""
    r = rigid_transform(theta, (0.0, 0.0, 0.0))[:3, :3]
    return math.degrees(math.acos(min(1.0, max(-1.0, (float(np.trace(r)) - 1.0) / 2.0))))


def _spacing(affine) -> np.ndarray:
    a = np.asarray(affine, dtype=np.float64)[:3, :3]
    return np.sqrt((a * a).sum(0))


def bin_range(ops, who: str, x, mask: str):
    """(lo, scale) of the float32 volume `x`: lo, hi its 0.5 and 99.5 percentile over its mask, scale = float32(BINS /
    (hi - lo)); PrepError naming `who` when hi <= lo or a bound is not finite."""
    count, stats = ops.prep_quantiles(x.reshape(1, -1), PERCENTILES, mask)
    n, stats = int(count.cpu().tolist()[0]), stats.cpu().numpy()
    if n < 2:
        raise prep.PrepError(f"{who}: --prep_register: {n} voxels inside the mask, the bin range needs two")
    lo, hi = (prep.percentile_value(n, q, stats[0, r, 0], stats[0, r, 1]) for r, q in enumerate(PERCENTILES))
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise prep.PrepError(f"{who}: --prep_register: the percentiles p{PERCENTILES[0]:.7g} = {lo} and "
                             f"p{PERCENTILES[1]:.7g} = {hi} over the mask give no bin range (needs finite lo < hi)")
    return lo, float(np.float32(BINS / (hi - lo)))


class Reference:
    """What the reference contributes to every registration of one subject, made once: per level (s, fbin)."""

    def __init__(self, ops, subject: str, name: str, x, affine, mask: str = "nonzero"):
        self.subject, self.name, self.mask = subject, name, mask
        self.affine = np.asarray(affine, dtype=np.float64)
        self.shape = tuple(int(n) for n in x.shape)
        self.spacing = _spacing(self.affine)
        bins = getattr(ops, "prep_bins", None) or partial(ops_register.prep_bins, ops)
        lo, scale = bin_range(ops, f"subject {subject}: {name}", x, mask)
        strides = [s for s in STRIDES if s == 1 or all(-(-n // s) >= MIN_SAMPLES for n in self.shape)]
        self.levels = []
        for s in strides:
            sig = prep.antialias_sigma(float(s))
            y = ops.prep_smooth(x[None], (sig, sig, sig), mask == "nonzero")[0] if prep.antialias_radius(sig) > 0 else x
            self.levels.append((s, bins(y, lo, scale, mask == "nonzero")))


def register_rigid(ops, ref: Reference, name: str, moving, a_src) -> Registered:
    """Register the float32 device volume `moving` (voxel-to-world `a_src`) onto `ref` by the rule above."""
    sn = ref.subject
    hist_of = getattr(ops, "prep_joint_hist", None) or partial(ops_register.prep_joint_hist, ops)
    lo, scale = bin_range(ops, f"subject {sn}: {name}", moving, ref.mask)
    unit = float(ref.spacing.min())                               # the finest reference spacing, mm
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64) * \
        (np.asarray(ref.shape, dtype=np.float64) - 1.0)
    centre = grid_centre(ref.affine, ref.shape)
    reach = max(float(np.linalg.norm(ref.affine[:3, :3] @ c + ref.affine[:3, 3] - centre)) for c in corners)
    reach = max(reach, unit)
    mov_spacing = _spacing(a_src)
    zero = (0.0,) * 6
    matrix = partial(rigid_matrix, sn, name, a_src, ref.affine, ref.shape)
    theta, evals, converged, before, value = zero, 0, True, 0.0, 0.0
    for s, fbin in ref.levels:
        sig = [prep.antialias_sigma(s * unit / float(m)) for m in mov_spacing]
        sig = [v if prep.antialias_radius(v) > 0 else 0.0 for v in sig]
        if s > 1 and max(prep.antialias_radius(v) for v in sig) > prep.ANTIALIAS_MAX_RADIUS:
            raise prep.PrepError(f"subject {sn}: {name}: --prep_register: at sample stride {s} its spacing "
                                 f"{prep._fmt(float(m) for m in mov_spacing)} against the reference's {unit:.7g} mm needs a "
                                 f"filter of radius {max(prep.antialias_radius(v) for v in sig)} voxels, more than "
                                 f"{prep.ANTIALIAS_MAX_RADIUS}: resample {name} to a coarser grid first")
        mov = ops.prep_smooth(moving[None], sig, ref.mask == "nonzero")[0] if s > 1 and any(v > 0 for v in sig) else moving

        def launch(thetas):
            h = hist_of(fbin, mov, np.stack([matrix(t) for t in thetas]), lo, scale, (s, s, s))
            return [a for a in h.cpu().numpy()]
        base = launch([zero])[0]
        evals += 1
        floor_total = int(base.sum()) / 2.0
        if s == 1:
            before = nmi(base)
        step, launches = 2.0 * s * unit, 0
        while step >= s * unit / 8.0:
            if launches == MAX_LAUNCHES:
                converged = False
                break
            cands = candidates(theta, step, step / reach)
            hists = launch(cands)
            launches += 1
            evals += 1
            scores = [nmi(h) if k == 0 or int(h.sum()) >= floor_total else -math.inf for k, h in enumerate(hists)]
            value = scores[0]
            best = max(range(len(cands)), key=lambda k: (scores[k], -k))
            if scores[best] > scores[0]:
                theta, value = cands[best], scores[best]
            else:
                step /= 2.0
    return Registered(tuple(theta), matrix(theta), before, value, evals, converged)
