"""The ``prep`` mission: source NIfTI scans to the data layout the ``ptq`` mission reads (data.py).

    python -m efficientq_amd.entrance prep --task brats --src_list cases.csv --data_dir out/data \
        [--split_dir out/split --round 1 --val_every 5] [--prep_mask nonzero|all] [--prep_window lo,hi|pLO,pHI|none] \
        [--prep_align MODALITY] [--prep_orient RAS] \
        [--prep_spacing d,h,w [--prep_antialias] [--prep_interp linear|cubic]] \
        [--prep_min_size d,h,w] [--prep_no_crop] [--access_type npy|npz]

``--src_list`` is a CSV with the header ``subject,<modality>,...[,seg]`` (the task's modalities, data.MODALITIES, in any
order) and one row per subject with one NIfTI path per column, relative to the CSV unless absolute; an empty ``seg``
cell is a subject without a label.  Per subject, on the device (csrc/prep.hip):

    align      --prep_align MODALITY: every other modality, and the label, whose header does not lie on the grid of
               MODALITY (the reference) is resampled onto it by the two affines as they stand, trilinear for the images,
               nearest for the label, 0 outside the scan's field of view (the rule below at ALIGN_COLUMNS;
               csrc/prep_align.hip); no registration, and no filter when the reference is the coarser grid
    reorient   --prep_orient CODE: the axes permuted and reversed (csrc/reorient.hip) so that array axis 0, 1, 2 runs
               towards the three letters of CODE (one each of R/L, A/P, S/I: RAS, LPS, SAR, ...), whatever orientation
               the scan's affine gives it; --prep_spacing and --prep_min_size then refer to the oriented axes
    window     --prep_window lo,hi: clip in place (lits: -200,250 unless ``none``; brats: none).  --prep_window pLO,pHI
               (p0.5,p99.5): every modality of every subject is clipped to a pair of its own percentiles over its own
               mask instead, and only inside that mask (the rule below at PercentileWindow; csrc/prep_quantile.hip)
    filter     --prep_antialias (with --prep_spacing): a separable Gaussian over the images on the source grid before
               they are down-sampled, per axis of factor f = target / source spacing > 1 with sigma = (f - 1) / 2 and
               the radius int(4 sigma + 0.5) (antialias_taps; csrc/prep_smooth.hip); the label is not touched
    resample   --prep_spacing d,h,w: trilinear for the images, nearest for the label; no filter before down-sampling
               unless --prep_antialias asks for one.  --prep_interp cubic: the images by cubic B-spline interpolation
               instead (the rule below at CUBIC_POLE; csrc/prep_spline.hip), on the same grid; the window is applied
               once more after it, since a cubic spline overshoots (a percentile window with the bounds found on the
               source grid); the label stays nearest
    pass 1     the box of the union of the modalities' masks, per modality the count and the sum over its own mask
               (--prep_mask nonzero: x != 0, the brats default; all: every voxel, the lits default)
    pass 2     per modality the squared deviations from the mean of pass 1; std = sqrt(sqdev / count)
    pass 3     (x - mean) / std inside the mask and exactly 0 outside it, cropped to the box

and the files ``data_dir/<modality>/<subject>.npy`` (float32), ``data_dir/seg/<subject>.npy`` (uint8), and at the end
``data_dir/sn_fn.txt``, ``data_dir/restore_shape_infokw.pickle`` and ``data_dir/prep.csv``, merged with what an earlier
run into the same ``data_dir`` left.  Without ``--prep_spacing`` sn_fn.txt names the first modality's own source image,
so ``ptq --src_geom --save_nii`` writes maps that overlay the scan; with it the arrays live on a new grid, which
``data_dir/grid/<subject>.nii.gz`` (the union mask, uint8, with the grid's affine) records and sn_fn.txt names.  With
``--prep_orient`` the arrays do not share the scan's axes either: the grid image is written then too (for every subject,
also one that was oriented as asked already), and prep.csv gains the columns ``source_orient`` and ``orient``.
With ``--prep_antialias`` prep.csv gains the column ``antialias`` after all others: the sigmas of the three array axes
in voxels of the source grid, ``0 0 0`` for a subject no axis of which is down-sampled far enough to be filtered.
With ``--prep_interp cubic`` prep.csv gains the column ``interp`` (``cubic``) after all others, the anti-alias column
included.  With ``--prep_align`` prep.csv gains the columns ``align`` (the reference) and ``align_inside`` (per modality
in the task's order, then the label: the voxels of the reference grid inside that scan's field of view, the whole grid
for one that was not resampled) after ``interp``, and "the first modality" above is the reference: its shape, spacing,
affine and header are the subject's, and sn_fn.txt names its scan.  With ``--prep_window pLO,pHI`` prep.csv gains
``<modality>_win_lo`` and ``<modality>_win_hi`` per modality (``repr(float)``) after all others, ``interp`` and the
align columns included.  A NaN or an Inf in a scan is carried along whole lines by the
spline's recursions; the check of the standard deviation then stops the run at that subject.
``--split_dir --val_every K`` also writes ``split_dir/round<R>/{train,val}.txt``.

What the headers decide (the list itself, shapes and affines within a subject, a grid smaller than --prep_min_size, a
split that already exists) is checked for every subject before anything is written.  What only the voxels decide (an
empty mask, a constant modality, a percentile bound that is not finite or, with the mask ``nonzero``, exactly 0) stops
the run at that subject: none of its files and none of the files written at the end exist then.  The next subject's
files are read and gunzipped by one background thread while the device works (read_subjects).  The nine --prep_*
options are one record, PrepOptions (parse_options), which the ``predict`` mission parses and uses the same way.
There is no CPU path: `ops` is hip_ops.get_ops(device) unless a caller passes its own.
"""
from __future__ import annotations

import csv
import math
import os
import os.path as P
import pickle
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from contextlib import closing
from functools import partial
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import data as D
from . import nifti
from . import ops_align

GRID_DIR = "grid"
PREP_CSV = "prep.csv"
MASK_DEFAULT = {"brats": "nonzero", "lits": "all"}
WINDOW_DEFAULT = {"brats": None, "lits": (-200.0, 250.0)}
AFFINE_TRANSLATION_TOL_MM = 1e-3
AFFINE_LINEAR_RTOL = 1e-4


class PrepError(SystemExit):
    """A run that cannot go on; the message names the row or the subject."""


# ---- the geometry of the steps (host, no device) ------------------------------------------------------------------------
def resample_extent(extent: int, factor: float) -> int:
    """Output extent of an axis: max(1, round(extent / factor)) with Python's round on the fp64 quotient (ties to even)."""
    return max(1, int(round(float(extent) / float(factor))))


def resample_affine(affine: np.ndarray, factors: Sequence[float]) -> np.ndarray:
    """A' = A [[diag(f), (f - 1) / 2], [0, 1]]: output voxel o lies at source coordinate (o + 0.5) f - 0.5."""
    f = np.asarray(factors, dtype=np.float64)
    m = np.eye(4)
    m[:3, :3] = np.diag(f)
    m[:3, 3] = (f - 1.0) / 2.0
    return np.asarray(affine, dtype=np.float64) @ m


def widen_box(pmin: Sequence[int], pmax: Sequence[int], grid: Sequence[int], min_size: Sequence[int]):
    """The box pmin:pmax widened to at least `min_size` per axis: symmetrically, the extra voxel of an odd widening on
    the low side, then shifted back into the grid.  The grid must hold `min_size`."""
    lo, hi = [], []
    for a, b, n, m in zip(pmin, pmax, grid, min_size):
        a, b, n, m = int(a), int(b), int(n), int(m)
        if m > n:
            raise ValueError(f"grid extent {n} smaller than the least size {m}")
        need = m - (b - a)
        if need > 0:
            a -= (need + 1) // 2
            b += need // 2
            if a < 0:
                a, b = 0, b - a
            if b > n:
                a, b = a - (b - n), n
        lo.append(a)
        hi.append(b)
    return tuple(lo), tuple(hi)


def _triple(s, what: str, cast=float) -> tuple:
    try:
        v = tuple(cast(x) for x in (s.split(",") if isinstance(s, str) else s))
    except (TypeError, ValueError):
        v = ()
    if len(v) != 3 or not all(math.isfinite(x) and x > 0 for x in v):
        raise PrepError(f"{what} {s!r}: needs three positive numbers d,h,w")
    return v


# ---- the percentile window (host, no device) ------------------------------------------------------------------------------
# The one definition of the rule of --prep_window pLO,pHI; include/effq_hip.h (effq_prep_quantiles) restates it.
# 1 The step runs where the absolute window runs: after the reorientation, before the filter and the resampling.
# 2 For modality c take the n voxels of its own mask (--prep_mask nonzero: x != 0, a NaN is inside; all: every voxel)
#   and sort them ascending: -Inf first, -0.0 counted as +0.0, every NaN after +Inf.
# 3 The value of percentile q, in fp64 with the product first: h = (n - 1) * q / 100, k = floor(h), a = sorted[k],
#   b = sorted[min(k + 1, n - 1)]; v = a when a == b, else a + (h - k) * (b - a); the bound is the float32 nearest v
#   (percentile_value).  That is numpy's default `linear` method, up to the rounding of h.
# 4 The voxels inside the mask are clipped to [lo_c, hi_c]; those outside it are left alone: with `nonzero` an exact zero
#   stays an exact zero, so the background and the crop box stay what they were.  A NaN stays a NaN.
# 5 The run stops at the subject (PrepError naming the subject, the modality and the bound; none of its files are
#   written) when a modality has fewer than two voxels inside its mask, when a bound is not finite, and, with `nonzero`,
#   when a bound comes to exactly 0: it would move voxels out of the mask.
# 6 With --prep_interp cubic the window applied once more after the resampling is this masked window with the same
#   bounds, found once, on the source grid.
class PercentileWindow:
    """--prep_window pLO,pHI: the percentiles 0 <= lo_q < hi_q <= 100 every modality is clipped to, over its own mask."""
    __slots__ = ("lo_q", "hi_q")

    def __init__(self, lo_q: float, hi_q: float):
        self.lo_q, self.hi_q = float(lo_q), float(hi_q)

    def __eq__(self, other):
        return isinstance(other, PercentileWindow) and (self.lo_q, self.hi_q) == (other.lo_q, other.hi_q)

    def __hash__(self):
        return hash((self.lo_q, self.hi_q))

    def __repr__(self):
        return f"PercentileWindow({self.lo_q!r}, {self.hi_q!r})"

    def __str__(self):      # as predict.csv spells it: p0.5 p99.5
        return f"p{self.lo_q:.7g} p{self.hi_q:.7g}"


WINDOW_FORMS = "lo,hi, pLO,pHI (percentiles, 0 <= LO < HI <= 100) or none"


def window_columns(mods: Sequence[str]) -> List[str]:
    """prep.csv, only with --prep_window pLO,pHI: the bounds of every modality, after all other columns."""
    return [f"{m}_win_{k}" for m in mods for k in ("lo", "hi")]


def percentile_value(n: int, q: float, a, b) -> float:
    """The host half of the rule: the float32 bound from the order statistics a = sorted[k] and b = sorted[min(k + 1,
    n - 1)], k = floor((n - 1) * q / 100), that the device found (hip_ops.prep_quantiles)."""
    h = float(int(n) - 1) * float(q) / 100.0
    k = math.floor(h)
    a, b = float(a), float(b)
    v = a if a == b else a + (h - k) * (b - a)
    return float(np.float32(v))


def parse_window(s, task: str):
    """None, the pair (lo, hi) of an absolute window, or a PercentileWindow."""
    if s is None:
        return WINDOW_DEFAULT[task]
    if isinstance(s, str) and s.strip().lower() in ("none", ""):
        return None
    parts = s.split(",") if isinstance(s, str) else s
    try:
        pct = [isinstance(x, str) and x.strip().lower().startswith("p") for x in parts]
    except TypeError:
        pct = []
    if any(pct):
        if len(pct) != 2:
            raise PrepError(f"--prep_window {s!r}: needs {WINDOW_FORMS}")
        if not all(pct):
            raise PrepError(f"--prep_window {s!r}: one bound is a percentile and the other is not: needs {WINDOW_FORMS}")
        try:
            lo, hi = (float(x.strip()[1:]) for x in parts)
        except ValueError:
            raise PrepError(f"--prep_window {s!r}: needs {WINDOW_FORMS}")
        if not all(math.isfinite(v) and 0.0 <= v <= 100.0 for v in (lo, hi)):
            raise PrepError(f"--prep_window {s!r}: a percentile lies within 0 and 100: needs {WINDOW_FORMS}")
        if not lo < hi:
            raise PrepError(f"--prep_window {s!r}: pLO must lie below pHI: needs {WINDOW_FORMS}")
        return PercentileWindow(lo, hi)
    try:
        lo, hi = (float(x) for x in parts)
    except (TypeError, ValueError):
        raise PrepError(f"--prep_window {s!r}: needs {WINDOW_FORMS}")
    if not lo <= hi:
        raise PrepError(f"--prep_window {s!r}: lo must not exceed hi")
    return lo, hi


# ---- the anti-alias filter before down-sampling (host, no device) -------------------------------------------------------
# The one definition of the rule of --prep_antialias; include/effq_hip.h (effq_prep_smooth) restates it.
ANTIALIAS_TRUNCATE = 4.0        # scipy.ndimage.gaussian_filter1d's default
ANTIALIAS_MAX_RADIUS = 32       # EFFQ_PREP_SMOOTH_MAX_RADIUS of include/effq_hip.h
ANTIALIAS_COLUMNS = ["antialias"]      # prep.csv and predict.csv, only with --prep_antialias


def antialias_sigma(factor: float) -> float:
    """The Gaussian's sigma, in source voxels, for an axis resampled by `factor` = target spacing / source spacing:
    (factor - 1) / 2 when the axis is down-sampled (skimage.transform.rescale(anti_aliasing=True)), 0 otherwise."""
    f = float(factor)
    return (f - 1.0) / 2.0 if f > 1.0 else 0.0


def antialias_radius(sigma: float) -> int:
    """The taps reach from -r to r with r = int(truncate sigma + 0.5); an axis with r = 0 is not filtered."""
    return int(ANTIALIAS_TRUNCATE * float(sigma) + 0.5)


def antialias_taps(sigma: float) -> np.ndarray:
    """The r + 1 taps g_0 ... g_r (g_-k = g_k) of one axis as the device takes them: exp(-k^2 / (2 sigma^2)) in fp64,
    normalised so that the 2 r + 1 taps sum to 1, then rounded to float32 and not normalised again.  r = 0: [1]."""
    r = antialias_radius(sigma)
    if r == 0:
        return np.ones(1, dtype=np.float32)
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    g /= g.sum()
    return g[r:].astype(np.float32)


# ---- cubic B-spline resampling (host, no device) -----------------------------------------------------------------------
# The one definition of the rule of --prep_interp cubic; include/effq_hip.h (effq_prep_resample_cubic) restates it.
# 1 Prefilter (the B-spline coefficient transform), along each array axis of extent n >= 2, in fp64: the coefficients c
#   solve (c[k-1] + 4 c[k] + c[k+1]) / 6 = x[k] with the whole-sample mirror c[-1] = c[1], c[n] = c[n-2] (scipy's
#   mode='mirror'), by the recursion with the pole z = CUBIC_POLE and the gain CUBIC_GAIN:
#     c+[0] = 6 sum_{k=0}^{2n-3} z^k xm[k] / (1 - z^(2n-2)), xm the mirrored line of period 2n - 2: the exact sum, no
#       truncated horizon;  c+[k] = 6 x[k] + z c+[k-1];
#     c[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]);  c[k] = z (c[k+1] - c+[k]).
#   An axis of extent 1 is not filtered; all three axes are filtered, one with factor 1 included (it is the same spline).
# 2 Evaluation: output index o of an axis sits at s = (o + 0.5) f - 0.5 in fp64, clamped to [0, n - 1] (the coordinate of
#   the trilinear path); i0 = floor(s), t = s - i0, and the weights on c[i0-1 .. i0+2] are cubic_weights(t), the indices
#   -1 and n mirrored; on an axis of extent 1 the one coefficient has weight 1.  The 64 terms are summed in fp64, w
#   innermost, then h, then d, and the sum is rounded to float32 once.  The output extents and the grid's affine are
#   resample_extent and resample_affine: the grid does not change with the order.
# 3 With --prep_mask nonzero (zero_keep) an output voxel is exactly 0 when every source voxel of its trilinear footprint
#   is exactly 0 (per axis i0 and i0 + 1, the second only when s > i0 and i0 < n - 1; a NaN is not 0): the prefilter has
#   infinite support, and the calibration takes exact 0 as background.  The body cannot grow past what the trilinear
#   step reaches.  --prep_mask all: nothing is kept.
# 4 With a --prep_window in force the window is applied once more after the resampling: values lie in [lo, hi] (a
#   percentile window: inside the mask, with the bounds found on the source grid).
# 5 A NaN or an Inf is carried along whole lines; the check of the standard deviation stops the run at that subject.
CUBIC_POLE = math.sqrt(3.0) - 2.0
CUBIC_GAIN = 6.0
INTERP_ORDERS = ("linear", "cubic")
INTERP_COLUMNS = ["interp"]      # prep.csv and predict.csv, only with --prep_interp cubic


def cubic_weights(t: float) -> Tuple[float, float, float, float]:
    """The cubic B-spline's weights on the coefficients i0 - 1, i0, i0 + 1, i0 + 2 at the offset t = s - i0 in [0, 1)."""
    t = float(t)
    return ((1.0 - t) ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0,
            (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0, t ** 3 / 6.0)


# ---- orientation (host, no device) ---------------------------------------------------------------------------------------
# NIfTI world axes: +x = R, +y = A, +z = S.  A code names, per array axis 0, 1, 2 (D, H, W = NIfTI i, j, k), the
# anatomical direction the axis runs towards.
ORIENT_LETTERS = {"R": (0, 1), "L": (0, -1), "A": (1, 1), "P": (1, -1), "S": (2, 1), "I": (2, -1)}
_LETTER_OF = {v: k for k, v in ORIENT_LETTERS.items()}


def parse_orient(code) -> Optional[str]:
    """The code of --prep_orient in capitals, or None when the switch is absent; a code that is not understood is
    refused by name."""
    if code is None:
        return None
    text = str(code).strip().upper()
    why = None
    if len(text) != 3:
        why = f"{len(text)} letters"
    elif any(c not in ORIENT_LETTERS for c in text):
        why = f"the letter {next(c for c in text if c not in ORIENT_LETTERS)!r} is none of R, L, A, P, S, I"
    elif len({ORIENT_LETTERS[c][0] for c in text}) != 3:
        why = "two letters of one pair"
    if why:
        raise PrepError(f"--prep_orient {code!r}: {why}: needs three letters, one each of R/L, A/P and S/I, in any order "
                        f"(RAS, LPS, SAR, ...)")
    return text


def orient_code(world_axis: Sequence[int], sign: Sequence[int]) -> str:
    """The three letters of an orientation: array axis a runs along world axis world_axis[a] in the direction sign[a]."""
    return "".join(_LETTER_OF[(int(w), 1 if s > 0 else -1)] for w, s in zip(world_axis, sign))


def scan_orientation(affine) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """(world_axis, sign) of a voxel-to-world affine: array axis a runs nearest to world axis world_axis[a] (0 = x, R; 1 =
    y, A; 2 = z, S), towards + (sign 1) or - (sign -1); orient_code(...) spells it.  The columns of the 3 x 3 part are
    normalised to unit length; the row of the largest absolute component decides.  Refused (PrepError with the cause;
    the caller names the subject): a column of zero or non-finite length, a column whose largest component does not
    strictly exceed its second largest (a 45 degree oblique), two array axes nearest to the same world axis."""
    m = np.asarray(affine, dtype=np.float64)[:3, :3]
    world, sign = [], []
    for a in range(3):
        col = m[:, a]
        length = float(np.sqrt((col * col).sum()))
        if not math.isfinite(length) or length <= 0.0:
            raise PrepError(f"the affine's column {a} has length {length}: array axis {a} has no direction")
        c = np.abs(col / length)
        order = np.argsort(-c, kind="stable")
        if not c[order[0]] > c[order[1]]:
            raise PrepError(f"the affine's column {a} lies at 45 degrees between two world axes (components "
                            f"{_fmt(float(v) for v in col / length)}): no nearest anatomical axis")
        world.append(int(order[0]))
        sign.append(1 if col[order[0]] > 0 else -1)
    if sorted(world) != [0, 1, 2]:
        raise PrepError(f"the affine maps two array axes nearest to the same world axis (axes 0, 1, 2 -> world "
                        f"{tuple(world)}): it is sheared too far to name an orientation")
    return tuple(world), tuple(sign)


def orient_plan(world_axis: Sequence[int], sign: Sequence[int], code: str, shape: Sequence[int]):
    """(src_axis, flip, out_shape) that turn a scan of orientation (world_axis, sign) and `shape` into `code`: output
    axis p is source axis src_axis[p], reversed iff flip[p]:  y[n0, n1, n2] = x[s] with
    s[src_axis[p]] = shape[src_axis[p]] - 1 - n_p if flip[p] else n_p."""
    src, flip = [], []
    for letter in parse_orient(code):
        w, s = ORIENT_LETTERS[letter]
        a = list(world_axis).index(w)
        src.append(a)
        flip.append(int(sign[a]) != s)
    return tuple(src), tuple(flip), tuple(int(shape[a]) for a in src)


def orient_inverse(src_axis: Sequence[int], flip: Sequence[bool]):
    """(inv_src_axis, inv_flip): the plan that, applied to the output of (src_axis, flip), gives the input back."""
    inv = [list(src_axis).index(a) for a in range(3)]
    return tuple(inv), tuple(bool(flip[p]) for p in inv)


def orient_is_identity(src_axis: Sequence[int], flip: Sequence[bool]) -> bool:
    return tuple(src_axis) == (0, 1, 2) and not any(flip)


def orient_affine(affine, src_axis: Sequence[int], flip: Sequence[bool], shape: Sequence[int]) -> np.ndarray:
    """A T with T the 4 x 4 integer matrix of the plan's index map (output index -> source index, `shape` the source's):
    every voxel keeps its world position."""
    t = np.zeros((4, 4))
    t[3, 3] = 1.0
    for p, (a, f) in enumerate(zip(src_axis, flip)):
        t[a, p] = -1.0 if f else 1.0
        t[a, 3] = float(int(shape[a]) - 1) if f else 0.0
    return np.asarray(affine, dtype=np.float64) @ t


# ---- alignment by the headers (host, no device) -------------------------------------------------------------------------
# The one definition of the rule of --prep_align MODALITY; include/effq_hip.h (effq_prep_align) restates the device half.
# 1 MODALITY names the reference.  A modality, or the label, whose header passes check_same_grid against the reference's is
#   used as it is, bit for bit.  For any other the plan holds M = inv(A_src) A_ref (align_matrix: 3 x 4, fp64), which maps
#   a voxel index (d, h, w, 1) of the reference grid to voxel coordinates of the source.  The affines are believed as
#   they stand: this is no registration.
# 2 The step comes first, on the scans' own axes, before --prep_orient; everything after it sees one grid.
# 3 Per voxel of the reference grid and source axis a, in fp64 and in this order:
#   s_a = ((M[a][0] d + M[a][1] h) + M[a][2] w) + M[a][3].  The voxel is inside the source's field of view when
#   -0.5 <= s_a < n_a - 0.5 on all three axes (n the source extent); outside it the result is +0.0, the background of
#   --prep_mask nonzero, or label 0.  `<` at the upper end: every source voxel owns the half voxel on either side of its
#   centre, the lower end included and the upper excluded, so the nearest index floor(s_a + 0.5) never reaches n_a.
# 4 Inside, an image is trilinear: c = clamp(s_a, 0, n_a - 1) (the edge replicated over the outer half voxel), i0 =
#   floor(c), i1 = min(i0 + 1, n_a - 1), l1 = float32(c - i0), l0 = 1 - l1 in fp32, the eight neighbours combined in fp32 in
#   the order of --prep_spacing's trilinear step.  The label takes the voxel floor(s_a + 0.5), at most n_a - 1.
# 5 Nothing is filtered when the reference grid is the coarser one, and --prep_interp cubic and --prep_antialias keep
#   their meaning: the --prep_spacing step only.
# 6 The run stops before anything is written at an A_src with an entry that is not finite or a 3 x 3 part of determinant
#   0, and at an M with an entry that is not finite; it stops at the subject when no voxel of the reference grid lies
#   inside a resampled scan.
ALIGN_COLUMNS = ["align", "align_inside"]      # prep.csv and predict.csv, only with --prep_align


def align_switch(args, task: str) -> Optional[str]:
    """--prep_align of `args` (or the YAML key): the reference modality, None when the switch is absent; anything but one
    of the task's modalities is refused by name."""
    ref = getattr(args, "prep_align", None)
    if ref is None:
        return None
    if not isinstance(ref, str) or ref.strip() not in D.MODALITIES[task]:
        raise PrepError(f"--prep_align {ref!r}: one of {', '.join(D.MODALITIES[task])}")
    return ref.strip()


def align_matrix(subject: str, name: str, a_src, a_ref) -> np.ndarray:
    """M = inv(A_src) A_ref as 3 x 4 fp64 (numpy.linalg.solve(A_src, A_ref)[:3]): reference voxel indices (d, h, w, 1) to
    voxel coordinates of the source `name`; step 6 of the rule refuses by subject and modality."""
    who = f"subject {subject}: --prep_align: {name}"
    a, r = np.asarray(a_src, dtype=np.float64), np.asarray(a_ref, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise PrepError(f"{who}: its affine holds an entry that is not finite")
    with np.errstate(all="ignore"):
        if np.linalg.det(a[:3, :3]) == 0.0:
            raise PrepError(f"{who}: the 3 x 3 part of its affine has determinant 0: its voxels have no place in the "
                            f"world")
        try:
            m = np.linalg.solve(a, r)[:3]
        except np.linalg.LinAlgError as e:
            raise PrepError(f"{who}: its affine cannot be inverted: {e}") from e
    if not np.all(np.isfinite(m)):
        raise PrepError(f"{who}: the matrix from the reference's grid to its own holds an entry that is not finite")
    return np.ascontiguousarray(m)


# ---- the source list ---------------------------------------------------------------------------------------------------
def read_src_list(path: str, task: str) -> List[dict]:
    """The rows of --src_list, sorted by subject: {subject, images: {modality: path}, seg: path or None}.  Everything the
    list alone decides is refused here, naming the row."""
    mods = D.MODALITIES[task]
    base = P.dirname(P.abspath(path))
    with open(path, "r", newline="") as f:
        rows = [r for r in csv.reader(f) if any(c.strip() for c in r)]
    if not rows:
        raise PrepError(f"--src_list {path}: empty")
    head = [c.strip() for c in rows[0]]
    want = set(mods)
    if head[0] != "subject" or len(set(head)) != len(head) or set(head[1:]) - {D.LABEL_MODALITY} != want \
            or len(head) not in (1 + len(mods), 2 + len(mods)):
        raise PrepError(f"--src_list {path}: row 1: columns {head}, needs subject,{','.join(mods)}[,{D.LABEL_MODALITY}] "
                        f"(each once)")
    out, seen = [], set()
    for i, r in enumerate(rows[1:], start=2):
        cells = [c.strip() for c in r] + [""] * (len(head) - len(r))
        if len(cells) != len(head):
            raise PrepError(f"--src_list {path}: row {i}: {len(r)} cells for {len(head)} columns")
        rec = dict(zip(head, cells))
        sn = rec["subject"]
        if not sn or "," in sn or "/" in sn or os.sep in sn or (os.altsep and os.altsep in sn) or sn in (".", ".."):
            raise PrepError(f"--src_list {path}: row {i}: subject name {sn!r} is empty or holds a comma or a path separator")
        if sn in seen:
            raise PrepError(f"--src_list {path}: row {i}: subject {sn} is listed twice")
        seen.add(sn)
        entry = {"subject": sn, "images": {}, "seg": None, "row": i}
        for col in head[1:]:
            cell = rec[col]
            if not cell:
                if col == D.LABEL_MODALITY:
                    continue
                raise PrepError(f"--src_list {path}: row {i} (subject {sn}): no path for {col}")
            full = cell if P.isabs(cell) else P.join(base, cell)
            if not P.isfile(full):
                raise PrepError(f"--src_list {path}: row {i} (subject {sn}): {col}: {full} is missing")
            if "," in full or "\n" in full:
                raise PrepError(f"--src_list {path}: row {i} (subject {sn}): {col}: a path with a comma cannot be named "
                                f"in {D.SN_FN_FILE}")
            if col == D.LABEL_MODALITY:
                entry["seg"] = full
            else:
                entry["images"][col] = full
        out.append(entry)
    if not out:
        raise PrepError(f"--src_list {path}: no subject")
    return sorted(out, key=lambda e: e["subject"])


def check_same_grid(subject: str, first: dict, other: dict, name: str) -> None:
    """`other` (a header: shape, affine) must lie on the grid of the subject's first modality."""
    if tuple(first["shape"][:3]) != tuple(other["shape"][:3]):
        raise PrepError(f"subject {subject}: {name} has shape {tuple(other['shape'][:3])}, the first modality "
                        f"{tuple(first['shape'][:3])}")
    a, b = np.asarray(first["affine"], dtype=np.float64), np.asarray(other["affine"], dtype=np.float64)
    dt = float(np.abs(a[:3, 3] - b[:3, 3]).max())
    scale = float(np.abs(a[:3, :3]).max())
    dl = float(np.abs(a[:3, :3] - b[:3, :3]).max())
    if dt > AFFINE_TRANSLATION_TOL_MM or dl > AFFINE_LINEAR_RTOL * scale:
        raise PrepError(f"subject {subject}: the affine of {name} differs from the first modality's (translation by "
                        f"{dt:.4g} mm, 3 x 3 part by {dl:.4g})")


def antialias_switch(args, spacing) -> bool:
    """--prep_antialias of `args` (or the YAML key); it filters ahead of the resampling, so without --prep_spacing it is
    refused by name."""
    on = bool(getattr(args, "prep_antialias", False))
    if on and spacing is None:
        raise PrepError("--prep_antialias filters the images before --prep_spacing down-samples them: it needs "
                        "--prep_spacing d,h,w")
    return on


def interp_switch(args, spacing) -> str:
    """--prep_interp of `args` (or the YAML key): 'linear' (also when absent) or 'cubic'; any other value is refused by
    name, and so is cubic without --prep_spacing, since it is the resampling that interpolates."""
    order = getattr(args, "prep_interp", None)
    order = "linear" if order is None else str(order).strip().lower()
    if order not in INTERP_ORDERS:
        raise PrepError(f"--prep_interp {getattr(args, 'prep_interp', None)!r}: linear or cubic")
    if order == "cubic" and spacing is None:
        raise PrepError("--prep_interp cubic is how --prep_spacing resamples the images: it needs --prep_spacing d,h,w")
    return order


class _Plan:
    """What the headers of one subject decide."""

    def __init__(self, entry: dict, mods: Sequence[str], spacing, min_size, orient: Optional[str] = None,
                 antialias: bool = False, interp: str = "linear", align: Optional[str] = None):
        sn = self.subject = entry["subject"]
        self.interp = interp if spacing is not None else "linear"      # how the images are resampled (--prep_interp)
        self.window_bounds = None       # --prep_window pLO,pHI: (lo, hi) per modality, set by process_subject
        self.entry = entry
        heads = {}
        for name, path in list(entry["images"].items()) + ([(D.LABEL_MODALITY, entry["seg"])] if entry["seg"] else []):
            try:
                h = nifti.read_geometry(path)
            except (OSError, ValueError, EOFError) as e:
                raise PrepError(f"subject {sn}: {name}: cannot read {path}: {e}") from e
            if len(h["shape"]) > 3 and any(n != 1 for n in h["shape"][3:]):
                raise PrepError(f"subject {sn}: {name}: {path} has shape {h['shape']}, only 3-D images are read")
            if h["datatype"] not in nifti.IMAGE_DATATYPES:
                raise PrepError(f"subject {sn}: {name}: {path} has datatype {h['datatype']}, one of "
                                f"{sorted(nifti.IMAGE_DATATYPES)} is read")
            heads[name] = h
        # --prep_align: the reference stands where the first modality stands without the switch; a header on another grid is
        # no refusal then but a matrix (align_matrix) and the source's own shape
        self.ref = align if align is not None else mods[0]
        self.align = {}                 # name -> (M, source shape) of what is resampled; empty without --prep_align
        self.align_inside = None        # per modality, then the label: set by process_subject under --prep_align
        self.shapes = {name: tuple(int(n) for n in h["shape"][:3]) for name, h in heads.items()}
        first = heads[self.ref]
        for name, h in heads.items():
            if name == self.ref:
                continue
            if align is None:
                check_same_grid(sn, first, h, name)
                continue
            m = align_matrix(sn, name, h["affine"], first["affine"])      # refused here also when the grids would pass
            try:
                check_same_grid(sn, first, h, name)
            except PrepError:
                self.align[name] = (m, self.shapes[name])
        self.source_shape = tuple(int(n) for n in first["shape"][:3])
        self.source_spacing = tuple(first["spacing"])
        self.affine = first["affine"]
        self.header = first             # nifti.read_geometry of that modality: write_nifti(..., geometry=header)
        # --prep_orient: the scan's own code and the plan (src_axis, flip) that turns it into the target's; without the
        # switch the affine is not looked at (orient_code None) and the oriented values are the scan's own
        self.orient_code, self.orient = None, None
        self.oriented_shape, self.oriented_spacing, self.oriented_affine = self.source_shape, self.source_spacing, \
            self.affine
        if orient is not None:
            try:
                world, sign = scan_orientation(self.affine)
            except PrepError as e:
                raise PrepError(f"subject {sn}: --prep_orient {orient}: {e}") from e
            self.orient_code = orient_code(world, sign)
            src, flip, self.oriented_shape = orient_plan(world, sign, orient, self.source_shape)
            self.orient = (src, flip)
            self.oriented_spacing = tuple(self.source_spacing[a] for a in src)
            self.oriented_affine = orient_affine(self.affine, src, flip, self.source_shape)
        if spacing is None:
            self.factors, self.grid_shape, self.grid_spacing, self.grid_affine = None, self.oriented_shape, \
                self.oriented_spacing, self.oriented_affine
        else:
            if min(self.oriented_spacing) <= 0:
                raise PrepError(f"subject {sn}: source spacing {self.source_spacing} cannot be resampled")
            self.factors = tuple(t / s for t, s in zip(spacing, self.oriented_spacing))
            self.grid_shape = tuple(resample_extent(n, f) for n, f in zip(self.oriented_shape, self.factors))
            self.grid_spacing = tuple(spacing)
            self.grid_affine = resample_affine(self.oriented_affine, self.factors)
        # --prep_antialias: per oriented axis the sigma the images are filtered with before the resample, 0 where the axis
        # is not down-sampled or the radius comes to 0; without the switch nothing is filtered
        self.sigmas, self.radii = (0.0, 0.0, 0.0), (0, 0, 0)
        if antialias and self.factors is not None:
            self.radii = tuple(antialias_radius(antialias_sigma(f)) for f in self.factors)
            self.sigmas = tuple(antialias_sigma(f) if r > 0 else 0.0 for f, r in zip(self.factors, self.radii))
            for a, (f, r) in enumerate(zip(self.factors, self.radii)):
                if r > ANTIALIAS_MAX_RADIUS:
                    raise PrepError(f"subject {sn}: --prep_antialias: array axis {a} is down-sampled by {f:.7g} (spacing "
                                    f"{self.oriented_spacing[a]:.7g} to {spacing[a]:.7g}): the filter's radius of {r} "
                                    f"voxels exceeds {ANTIALIAS_MAX_RADIUS}")
        if any(g < m for g, m in zip(self.grid_shape, min_size)):
            raise PrepError(f"subject {sn}: grid of {self.grid_shape} is smaller than --prep_min_size "
                            f"{tuple(min_size)}: the validation's sliding window needs one whole patch")


def _load(entry: dict, mods: Sequence[str]):
    """Read one subject's files (the background thread): ({modality: array}, label or None), or the exception."""
    try:
        imgs = {m: nifti.read_image(entry["images"][m])[0] for m in mods}
        seg = None
        if entry["seg"]:
            lab = nifti.read_image(entry["seg"])[0]
            if lab.size and (np.any(lab != np.floor(lab)) or lab.min() < 0 or lab.max() > 255):
                raise ValueError(f"the label {entry['seg']} is not integral within 0 ... 255")
            seg = lab.astype(np.uint8)
        return imgs, seg
    except Exception as e:        # handed to the main thread, which names the subject
        return e


def read_subjects(plans: Sequence[_Plan], mods: Sequence[str], thread_name_prefix: str):
    """(plan, {modality: array}, label or None) per plan, in order: one background thread reads and gunzips the next
    subject's files while the caller works on this one.  A failed read is the PrepError naming its subject.  When the
    generator ends or is closed early the pending read is cancelled and the thread is gone."""
    pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix=thread_name_prefix)
    try:
        nxt = pool.submit(_load, plans[0].entry, mods)
        for i, plan in enumerate(plans):
            got = nxt.result()
            nxt = pool.submit(_load, plans[i + 1].entry, mods) if i + 1 < len(plans) else None
            if isinstance(got, Exception):
                raise PrepError(f"subject {plan.subject}: {got}") from got
            yield (plan,) + got
    finally:
        pool.shutdown(wait=True, cancel_futures=True)


# ---- the options prep and predict share --------------------------------------------------------------------------------
class PrepOptions(NamedTuple):
    """The nine --prep_* options, as the ``prep`` and the ``predict`` mission both take them (parse_options)."""
    mask: str                               # --prep_mask: nonzero | all
    window: object                          # --prep_window: None, (lo, hi) or a PercentileWindow
    spacing: Optional[tuple]                # --prep_spacing d,h,w
    min_size: tuple                         # --prep_min_size d,h,w
    no_crop: bool                           # --prep_no_crop
    orient: Optional[str] = None            # --prep_orient CODE
    antialias: bool = False                 # --prep_antialias
    interp: str = "linear"                  # --prep_interp linear | cubic
    align: Optional[str] = None             # --prep_align MODALITY

    def plan(self, entry: dict, mods: Sequence[str]) -> _Plan:
        return _Plan(entry, mods, self.spacing, self.min_size, self.orient, self.antialias, self.interp, self.align)

    def columns(self) -> List[str]:
        """The optional columns of prep.csv and predict.csv that both missions write, in their order."""
        return (ORIENT_COLUMNS if self.orient else []) + (ANTIALIAS_COLUMNS if self.antialias else []) + \
            (INTERP_COLUMNS if self.interp == "cubic" else []) + (ALIGN_COLUMNS if self.align else [])

    def row_values(self, plan: _Plan) -> dict:
        """One subject's values of columns()."""
        row = {}
        if self.orient:
            row.update(source_orient=plan.orient_code, orient=self.orient)
        if self.antialias:
            row.update(antialias=_fmt(plan.sigmas))
        if self.interp == "cubic":
            row.update(interp=self.interp)
        if self.align:
            row.update(align=self.align, align_inside=_fmt(plan.align_inside))
        return row

    def said(self, plan: _Plan, mods: Sequence[str]) -> str:
        """What the per-subject line says after the source shape: "(LPS -> RAS)" when the scan was turned, every
        modality's bounds of a percentile window, the filter's sigmas when any is above 0, "cubic", and what --prep_align
        resampled with its share of the reference grid."""
        said = f" ({plan.orient_code} -> {self.orient})" if self.orient and plan.orient_code != self.orient else ""
        if plan.window_bounds is not None:
            said += ", window " + ", ".join(f"{m} {lo:.7g} {hi:.7g}" for m, (lo, hi) in zip(mods, plan.window_bounds))
        if any(s > 0 for s in plan.sigmas):
            said += f", anti-alias sigma {_fmt(plan.sigmas)}"
        said += ", cubic" if plan.interp == "cubic" else ""
        if plan.align:
            names = list(mods) + [D.LABEL_MODALITY]
            voxels = float(np.prod(plan.source_shape))
            said += f", aligned to {self.align}: " + ", ".join(
                f"{m} {n / voxels:.2f}" for m, n in zip(names, plan.align_inside) if m in plan.align)
        return said


def parse_options(args, task: str, default_min_size=None) -> PrepOptions:
    """The PrepOptions of `args`, each value that is not understood refused by name in the order of the fields;
    `default_min_size` stands for an absent --prep_min_size (None: the task's patch, data.PATCH_DEFAULT)."""
    mask = getattr(args, "prep_mask", None) or MASK_DEFAULT[task]
    if mask not in ("nonzero", "all"):
        raise PrepError(f"--prep_mask {mask!r}: nonzero or all")
    window = parse_window(getattr(args, "prep_window", None), task)
    spacing = _triple(args.prep_spacing, "--prep_spacing") if getattr(args, "prep_spacing", None) else None
    if getattr(args, "prep_min_size", None):
        min_size = _triple(args.prep_min_size, "--prep_min_size", int)
    else:
        min_size = D.PATCH_DEFAULT[task] if default_min_size is None else default_min_size
    return PrepOptions(mask, window, spacing, min_size, bool(getattr(args, "prep_no_crop", False)),
                       parse_orient(getattr(args, "prep_orient", None)), antialias_switch(args, spacing),
                       interp_switch(args, spacing), align_switch(args, task))


# ---- the files ---------------------------------------------------------------------------------------------------------
def _replace(path: str, write) -> None:
    tmp = path + ".tmp"
    write(tmp)
    os.replace(tmp, path)


def _replace_text(path: str, text: str) -> None:
    def dump(p):
        with open(p, "w") as f:
            f.write(text)
    _replace(path, dump)


def _save_array(data_dir: str, modality: str, subject: str, access_type: str, a: np.ndarray) -> None:
    os.makedirs(P.join(data_dir, modality), exist_ok=True)
    if access_type == "npz":
        np.savez(P.join(data_dir, modality, f"{subject}.npz"), a)
    else:
        np.save(P.join(data_dir, modality, f"{subject}.npy"), a)


def _read_sn_fn_raw(data_dir: str) -> Dict[str, str]:
    out = {}
    path = P.join(data_dir, D.SN_FN_FILE)
    if P.isfile(path):
        with open(path, "r") as f:
            for line in f.read().splitlines():
                if line.strip() and line.count(",") == 1:
                    sn, fn = (s.strip() for s in line.split(","))
                    out[sn] = fn
    return out


def write_index_files(data_dir: str, sn_fn: Dict[str, str], restore: Dict[str, Optional[dict]], rows: List[dict],
                      header: List[str]) -> None:
    """sn_fn.txt, the restore pickle and prep.csv, each merged with the file an earlier run left (the newer entry wins,
    lines sorted by subject) and written through a temporary file and a rename."""
    names = dict(_read_sn_fn_raw(data_dir))
    names.update(sn_fn)
    _replace_text(P.join(data_dir, D.SN_FN_FILE), "".join(f"{sn},{names[sn]}\n" for sn in sorted(names)))
    kept = dict(D.read_restore_info(data_dir) or {})
    for sn, kw in restore.items():
        if kw is None:
            kept.pop(sn, None)
        else:
            kept[sn] = {k: tuple(int(v) for v in kw[k]) for k in ("pmin", "pmax", "shape")}
    if kept or P.isfile(P.join(data_dir, D.RESTORE_FILE)):
        def dump(p):
            with open(p, "wb") as f:
                pickle.dump({sn: kept[sn] for sn in sorted(kept)}, f, protocol=4)
        _replace(P.join(data_dir, D.RESTORE_FILE), dump)
    old = {}
    path = P.join(data_dir, PREP_CSV)
    if P.isfile(path):
        with open(path, "r", newline="") as f:
            r = list(csv.reader(f))
        if r and r[0] == header:
            old = {line[0]: line for line in r[1:] if line}
    for row in rows:
        old[row["subject"]] = [row[k] for k in header]

    def dump_csv(p):
        with open(p, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(header)
            w.writerows(old[sn] for sn in sorted(old))
    _replace(path, dump_csv)


def prep_csv_header(mods: Sequence[str]) -> List[str]:
    return ["subject", "source_shape", "source_spacing", "grid_shape", "grid_spacing", "pmin", "pmax"] + \
        [f"{m}_{k}" for m in mods for k in ("count", "mean", "std")]


ORIENT_COLUMNS = ["source_orient", "orient"]      # prep.csv and predict.csv, only with --prep_orient


def _fmt(v) -> str:
    return " ".join(f"{x:.7g}" if isinstance(x, float) else str(int(x)) for x in v)


# ---- one subject on the device -------------------------------------------------------------------------------------------
def percentile_bounds(ops, sn: str, x, mods: Sequence[str], mask: str, window: PercentileWindow):
    """(lo, hi) per modality of C x D x H x W `x` by the rule at PercentileWindow, or the PrepError of its step 5."""
    qs = (window.lo_q, window.hi_q)
    count, stats = ops.prep_quantiles(x.reshape(x.shape[0], -1), qs, mask)
    count, stats = count.cpu().tolist(), stats.cpu().numpy()
    bounds = []
    for c, m in enumerate(mods):
        n = int(count[c])
        if n < 2:
            raise PrepError(f"subject {sn}: modality {m}: {n} voxels inside the mask, the percentiles p{qs[0]:.7g} and "
                            f"p{qs[1]:.7g} of --prep_window need two")
        pair = tuple(percentile_value(n, q, stats[c, r, 0], stats[c, r, 1]) for r, q in enumerate(qs))
        for q, v in zip(qs, pair):
            if not math.isfinite(v):
                raise PrepError(f"subject {sn}: modality {m}: the bound p{q:.7g} of --prep_window is {v}: a window "
                                f"needs finite bounds")
            if mask == "nonzero" and v == 0.0:
                raise PrepError(f"subject {sn}: modality {m}: the bound p{q:.7g} of --prep_window is exactly 0: with "
                                f"--prep_mask nonzero it would move voxels out of the mask")
        bounds.append(pair)
    return bounds


def _apply_window(ops, plan, x, window, mask: str) -> None:
    """The window in place: the absolute one over every voxel, the percentile one per modality inside its mask."""
    if plan.window_bounds is not None:
        for c, (lo, hi) in enumerate(plan.window_bounds):
            ops.prep_window_mask(x[c], lo, hi, mask)
    elif window is not None:
        ops.prep_window(x, window[0], window[1])


def _aligned(ops, plan: _Plan, imgs: Dict[str, np.ndarray], seg: Optional[np.ndarray], mods: Sequence[str]):
    """--prep_align: (x, lab) on the reference's grid.  Each modality goes to the device alone and is copied, or aligned by
    its matrix, into its plane of the C x D x H x W tensor, the label likewise; plan.align_inside gets the voxels of the
    grid inside each one's field of view, and a resampled scan that covers none of them stops the run."""
    align = getattr(ops, "prep_align", None) or partial(ops_align.prep_align, ops)
    dev, grid = ops.device, plan.source_shape
    full = int(np.prod(grid))
    x = torch.empty((len(mods),) + grid, dtype=torch.float32, device=dev)
    lab = torch.empty((1,) + grid, dtype=torch.uint8, device=dev) if seg is not None else None
    names = list(mods) + ([D.LABEL_MODALITY] if seg is not None else [])
    counted = {}        # name -> the one-element device tensor of effq_prep_align; read once, after the last launch
    for name, host, plane in zip(names, [imgs[m] for m in mods] + [seg], list(x) + [lab[0] if lab is not None else None]):
        t = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
        if name in plan.align:
            t, counted[name] = align(t, plan.align[name][0], grid, nearest=name == D.LABEL_MODALITY)
        plane.copy_(t)
    got = dict(zip(counted, torch.cat([n.reshape(1) for n in counted.values()]).cpu().tolist())) if counted else {}
    plan.align_inside = [int(got.get(name, full)) for name in names]
    for name in names:
        if got.get(name, full) == 0:
            raise PrepError(f"subject {plan.subject}: --prep_align {plan.ref}: {name}: no voxel of the reference grid lies "
                            f"inside it; do the headers share a world?")
    return x, lab


# what process_subject returns, host arrays: arrays C x d x h x w float32, the label or None, the union mask of the grid or
# None, the box, and per modality the count, mean and std over its mask
Subject = namedtuple("Subject", "arrays label union pmin pmax count mean std")


def process_subject(ops, plan: _Plan, imgs: Dict[str, np.ndarray], seg: Optional[np.ndarray], mods: Sequence[str],
                    opts: PrepOptions) -> Subject:
    """The device pipeline of one subject under `opts` (its mask, window, min_size and no_crop; the plan holds what the
    other options decided)."""
    sn, mask, window = plan.subject, opts.mask, opts.window
    for m in mods:          # every array against its own header; without --prep_align they all say plan.source_shape
        if tuple(imgs[m].shape) != plan.shapes[m]:
            raise PrepError(f"subject {sn}: {m} holds an array of shape {tuple(imgs[m].shape)}, its header says "
                            f"{plan.shapes[m]}")
    if seg is not None and tuple(seg.shape) != plan.shapes[D.LABEL_MODALITY]:
        raise PrepError(f"subject {sn}: the label holds an array of shape {tuple(seg.shape)}, not "
                        f"{plan.shapes[D.LABEL_MODALITY]}")
    dev = ops.device
    if opts.align is None:
        x = torch.from_numpy(np.stack([imgs[m] for m in mods])).to(dev)
        lab = torch.from_numpy(seg[None]).to(dev) if seg is not None else None
    else:
        x, lab = _aligned(ops, plan, imgs, seg, mods)
    if plan.orient is not None and not orient_is_identity(*plan.orient):
        x = ops.prep_reorient(x, *plan.orient)
        if lab is not None:
            lab = ops.prep_reorient(lab, *plan.orient)
    plan.window_bounds = percentile_bounds(ops, sn, x, mods, mask, window) if isinstance(window, PercentileWindow) \
        else None
    _apply_window(ops, plan, x, window, mask)
    if plan.factors is not None:
        if any(r > 0 for r in plan.radii):       # --prep_antialias; the label is not filtered
            x = ops.prep_smooth(x, plan.sigmas, mask == "nonzero")
        if plan.interp == "cubic":       # --prep_interp cubic; the spline overshoots, so the window once more
            x = ops.prep_resample_cubic(x, plan.factors, plan.grid_shape, mask == "nonzero")
            _apply_window(ops, plan, x, window, mask)
        else:
            x = ops.prep_resample(x, plan.factors, plan.grid_shape)
        if lab is not None:
            lab = ops.prep_resample(lab, plan.factors, plan.grid_shape, nearest=True)
    bbox, count, total = ops.prep_bbox_moments(x, mask)
    bbox, count, total = bbox.cpu().tolist(), count.cpu().tolist(), total.cpu().tolist()
    if any(a > b for a, b in zip(bbox[:3], bbox[3:])):
        raise PrepError(f"subject {sn}: every voxel of every modality is zero: there is no body to crop to")
    for m, n in zip(mods, count):
        if n < 2:
            raise PrepError(f"subject {sn}: modality {m}: {n} voxels inside the mask, the standard deviation needs two")
    mean = [s / n for s, n in zip(total, count)]
    sqdev = ops.prep_sqdev(x, mean, mask).cpu().tolist()
    std = [math.sqrt(q / n) for q, n in zip(sqdev, count)]
    for m, s in zip(mods, std):
        if not s > 0.0 or not math.isfinite(s):
            raise PrepError(f"subject {sn}: modality {m}: standard deviation {s} over the mask: a constant (or "
                            f"non-finite) image cannot be standardised")
    if opts.no_crop:
        pmin, pmax = (0, 0, 0), tuple(plan.grid_shape)
    else:
        pmin, pmax = widen_box(bbox[:3], [b + 1 for b in bbox[3:]], plan.grid_shape, opts.min_size)
    y = ops.prep_standardise_crop(x, pmin, pmax, mean, std, mask)
    lab_out = ops.prep_crop_u8(lab, pmin, pmax)[0].cpu().numpy() if lab is not None else None
    on_new_grid = plan.factors is not None or plan.orient is not None        # the arrays left the scan's own axes
    union = ops.prep_union_mask(x, mask).cpu().numpy() if on_new_grid else None
    return Subject(y.cpu().numpy(), lab_out, union, pmin, pmax, count, mean, std)


# ---- the mission -------------------------------------------------------------------------------------------------------
def run(args, ops=None) -> List[dict]:
    """The `prep` mission of `args` (config.build_parser); returns the rows of prep.csv of this run.  `ops`: the object
    whose prep_* methods do the device work and whose `device` holds the tensors, hip_ops.get_ops(args.device) by
    default."""
    task = (getattr(args, "task", None) or "").lower()
    if task not in D.MODALITIES:
        raise PrepError(f"prep: --task {getattr(args, 'task', None)!r}, one of {', '.join(D.MODALITIES)}")
    if not getattr(args, "src_list", None) or not getattr(args, "data_dir", None):
        raise PrepError("prep: needs --src_list and --data_dir")
    mods = D.MODALITIES[task]
    opts = parse_options(args, task)
    access = getattr(args, "access_type", None) or "npy"
    if access not in D.ACCESS_TYPES:
        raise PrepError(f"--access_type {access!r}: one of {', '.join(D.ACCESS_TYPES)}")
    data_dir = args.data_dir

    # everything the list and the headers decide, before anything is written
    plans = [opts.plan(e, mods) for e in read_src_list(args.src_list, task)]
    split = None
    if getattr(args, "split_dir", None):
        k = getattr(args, "val_every", None)
        if k is None or int(k) < 1:
            raise PrepError("--split_dir: needs --val_every K (K >= 1): every K-th of the sorted subjects validates")
        split = P.join(args.split_dir, f"round{args.round}")
        for name in ("train.txt", "val.txt"):
            if P.exists(P.join(split, name)):
                raise PrepError(f"--split_dir: {P.join(split, name)} exists already: prep does not overwrite a split")
        k = int(k)
    if ops is None:
        from .hip_ops import get_ops
        ops = get_ops(torch.device("cuda", int(getattr(args, "device", 0) or 0)))

    os.makedirs(data_dir, exist_ok=True)
    sn_fn, restore, rows = {}, {}, []
    with closing(read_subjects(plans, mods, "effq-prep-read")) as subjects:       # a subject that fails ends the reads
        for plan, imgs, seg in subjects:
            sn = plan.subject
            y, lab, union, pmin, pmax, count, mean, std = process_subject(ops, plan, imgs, seg, mods, opts)
            for c, m in enumerate(mods):
                _save_array(data_dir, m, sn, access, y[c])
            if lab is not None:
                _save_array(data_dir, D.LABEL_MODALITY, sn, access, lab)
            if union is not None:
                os.makedirs(P.join(data_dir, GRID_DIR), exist_ok=True)
                nifti.write_nifti(P.join(data_dir, GRID_DIR, f"{sn}.nii.gz"), union, plan.grid_affine)
                sn_fn[sn] = f"{GRID_DIR}/{sn}.nii.gz"
            else:
                sn_fn[sn] = P.abspath(plan.entry["images"][plan.ref])
            cropped = tuple(y.shape[1:]) != tuple(plan.grid_shape)
            restore[sn] = {"pmin": pmin, "pmax": pmax, "shape": plan.grid_shape} if cropped else None
            row = {"subject": sn, "source_shape": _fmt(plan.source_shape), "source_spacing": _fmt(plan.source_spacing),
                   "grid_shape": _fmt(plan.grid_shape), "grid_spacing": _fmt(plan.grid_spacing), "pmin": _fmt(pmin),
                   "pmax": _fmt(pmax)}
            for c, m in enumerate(mods):
                row.update({f"{m}_count": str(int(count[c])), f"{m}_mean": repr(float(mean[c])),
                            f"{m}_std": repr(float(std[c]))})
            row.update(opts.row_values(plan))
            if plan.window_bounds is not None:
                for m, (lo, hi) in zip(mods, plan.window_bounds):
                    row.update({f"{m}_win_lo": repr(float(lo)), f"{m}_win_hi": repr(float(hi))})
            rows.append(row)
            print(f"[prep] {sn}: {_fmt(plan.source_shape)}{opts.said(plan, mods)} -> {_fmt(y.shape[1:])} at {_fmt(pmin)}")
    write_index_files(data_dir, sn_fn, restore, rows, prep_csv_header(mods) + opts.columns() +
                      (window_columns(mods) if isinstance(opts.window, PercentileWindow) else []))
    if split is not None:
        names = [p.subject for p in plans]
        val = names[k - 1::k]
        os.makedirs(split, exist_ok=True)
        for name, sns in (("train.txt", [s for s in names if s not in set(val)]), ("val.txt", val)):
            _replace_text(P.join(split, name), "".join(s + "\n" for s in sns))
    print(f"[prep] {len(rows)} subjects written to {data_dir}")
    return rows
