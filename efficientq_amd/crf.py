"""Refinement of a predicted map by a locally connected conditional random field on the scans (--crf of the ``predict``
mission): mean-field iterations of the Potts model with a truncated bilateral and a truncated spatial
kernel, as DeepMedic applied the dense form and ConvCRF the local one.  The one definition of the rule; everything per
voxel runs on the device (ops_crf; csrc/seg_crf.hip).  Agreement with another tool's numbers is not claimed.

Per subject, on the working grid, between the stitch and everything that reads the logits.

Inputs      v (C, D, H, W) fp32, the stitched logits; x (M, D, H, W) fp32, the standardised images the windows were cut
            from; s = (s_d, s_h, s_w), the working grid's spacing in mm.
Parameters  w_a, w_s >= 0, w_a + w_s <= 64: the appearance and smoothness weights in logit units (4, 1);
            theta_p > 0 mm (3), theta_i > 0 standard deviations (0.5), theta_s > 0 mm (1), each within 1e-18 ... 1e18;
            T = 1 ... 20 iterations (5).
            The defaults are not tuned on data: measure with the ``score`` mission.
Offsets     t != 0 with |t_a| <= r_a = min(3, floor(2 max(theta_p, theta_s) / s_a)); an axis with r_a = 0 is not linked,
            and a subject with all three radii 0 is refused.  Neighbours outside the volume contribute nothing.
Kernels     d2 = sum_a (s_a t_a)^2;  g_p(t) = exp(-d2 / 2 theta_p^2) / Z_p,  g_s(t) = exp(-d2 / 2 theta_s^2) / Z_s,  Z the
            sum over all offsets, borders notwithstanding: w_a + w_s is the largest message an interior voxel receives.
Pair        k(i, j) = w_a g_p(t) exp(-sum_m (x_m(i) - x_m(j))^2 / 2 theta_i^2) + w_s g_s(t),  j = i + t.
Softmax     (class ids)  H0 = v;  Q = softmax_c(H);  H'_i(c) = v_i(c) + sum_j k(i, j) Q_j(c).
Sigmoid     (--multi_label brats: every channel a binary field)  Q = sigmoid(H);  H'_i(c) = v_i(c) + sum_j k(i, j) (2 Q_j(c) - 1).
Not finite  a voxel whose C logits and M intensities are not all finite sends no message and keeps H = v.
Output      H after T iterations, and `changed`: the voxels whose decision differs between v and H (the first largest
            channel, or any channel's side of the decision threshold in force).
Not built   the fully connected CRF, a learned compatibility matrix, kernels in source-grid millimetres, radii above 3.
"""
from __future__ import annotations

import math
from collections import namedtuple

from . import _lib
from . import ops_crf
from . import prep

MAX_RADIUS = ops_crf.MAX_RADIUS
MAX_WEIGHT, MAX_ITERS = float(_lib.SEG_CRF_MAX_WEIGHT), _lib.SEG_CRF_MAX_ITERS
THETA_MIN, THETA_MAX = _lib.SEG_CRF_THETA_RANGE       # what effq_seg_crf takes: the folded constants stay normal numbers
CrfParams = namedtuple("CrfParams", "w_a w_s theta_p theta_i theta_s iters")
DEFAULTS = CrfParams(4.0, 1.0, 3.0, 0.5, 1.0, 5)
CSV_COLUMNS = ["crf", "crf_changed"]          # predict.csv, after the thresh column's place and before the post columns
QUALIFIERS = ("crf_w", "crf_theta", "crf_iters")
SWITCHES = ("crf",) + QUALIFIERS


def _floats(switch: str, value, n: int, form: str):
    parts = list(value) if isinstance(value, (list, tuple)) else str(value).split(",")
    try:
        got = tuple(float(v) for v in parts)
    except (TypeError, ValueError):
        got = ()
    if len(got) != n or not all(math.isfinite(v) for v in got):
        raise SystemExit(f"--{switch} {value!r}: {form}")
    return got


def crf_switches(args, mission=None):
    """None without --crf, else the CrfParams of --crf_w WA,WS / --crf_theta P,I,S / --crf_iters T (or the YAML keys
    `crf`, `crf_w`, `crf_theta`, `crf_iters`).  Every mission but predict refuses all four by name, the three that qualify
    --crf are refused without it, and a value that is not understood is refused by name (SystemExit), host only."""
    mission = mission or getattr(args, "mission", None)
    given = [k for k in SWITCHES if getattr(args, k, None) not in (None, False)]
    if mission != "predict":
        for switch in given:
            raise SystemExit(f"--{switch} refines the maps the predict mission writes, by a conditional random field on the "
                             f"scans: the {mission} mission has no such step, drop --{switch}")
        return None
    if "crf" not in given:
        for switch in given:
            raise SystemExit(f"--{switch} qualifies --crf, which is not given: add --crf or drop --{switch}")
        return None
    w_a, w_s = DEFAULTS[:2]
    if "crf_w" in given:
        form = f"WA,WS: the appearance and smoothness weights, both >= 0, WA + WS <= {MAX_WEIGHT:g}"
        w_a, w_s = _floats("crf_w", args.crf_w, 2, form)
        if min(w_a, w_s) < 0.0 or w_a + w_s > MAX_WEIGHT:
            raise SystemExit(f"--crf_w {args.crf_w!r}: {form}")
    thetas = DEFAULTS[2:5]
    if "crf_theta" in given:
        form = "P,I,S: the widths of the appearance kernel in mm and in standard deviations and of the smoothness kernel " \
               f"in mm, all > 0 (within {THETA_MIN:g} ... {THETA_MAX:g})"
        thetas = _floats("crf_theta", args.crf_theta, 3, form)
        if not all(THETA_MIN <= t <= THETA_MAX for t in thetas):
            raise SystemExit(f"--crf_theta {args.crf_theta!r}: {form}")
    iters = DEFAULTS.iters
    if "crf_iters" in given:
        t = args.crf_iters
        if isinstance(t, bool) or not str(t).strip().isdigit() or not 1 <= int(t) <= MAX_ITERS:
            raise SystemExit(f"--crf_iters {t!r}: the iterations, an integer of 1 ... {MAX_ITERS}")
        iters = int(t)
    return CrfParams(w_a, w_s, *thetas, iters)


def radii(spacing, params: CrfParams):
    """(r_d, r_h, r_w) of a grid with `spacing` in mm: min(MAX_RADIUS, floor(2 max(theta_p, theta_s) / s_a)), as
    effq_seg_crf computes them."""
    reach = 2.0 * max(params.theta_p, params.theta_s)
    return tuple(int(min(float(MAX_RADIUS), math.floor(reach / float(s)))) for s in spacing)


def column_text(params: CrfParams) -> str:
    """The `crf` column of predict.csv: w_a w_s theta_p theta_i theta_s T."""
    return " ".join("%g" % v for v in params)


def said(params: CrfParams) -> str:
    """The [predict] line at the start of a run with --crf."""
    tuned = "the defaults, which are not tuned on data" if params == DEFAULTS else "not checked against data here"
    return (f"--crf: the stitched logits are refined by {params.iters} mean-field iterations of a local conditional random "
            f"field on the standardised scans: w_a {params.w_a:g}, w_s {params.w_s:g}, theta_p {params.theta_p:g} mm, "
            f"theta_i {params.theta_i:g} sd, theta_s {params.theta_s:g} mm ({tuned}: measure what they buy with the score "
            f"mission)")


def linked_radii(sn: str, spacing, params: CrfParams):
    """The radii of subject `sn`'s working grid; a grid no axis of which is linked is refused naming the subject and the
    spacing (predict asks from the headers, before a scan is read)."""
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3 or not all(math.isfinite(s) and s > 0.0 for s in spacing):
        raise prep.PrepError(f"subject {sn}: --crf: the working grid's spacing {spacing} is not three finite lengths above 0")
    r = radii(spacing, params)
    if not any(r):
        raise prep.PrepError(f"subject {sn}: --crf: at the working spacing {prep._fmt(spacing)} mm no neighbour lies within "
                             f"2 max(theta_p, theta_s) = {2.0 * max(params.theta_p, params.theta_s):g} mm on any axis: "
                             f"nothing is linked; widen --crf_theta or drop --crf")
    return r


def refine(ops, sn: str, logits, images, spacing, mode: str, params: CrfParams, thresh: float = 0.0, step=None):
    """(H, changed, radii) of the (C, D, H, W) float32 device `logits` and the (M, D, H, W) float32 device `images` of
    subject `sn` on a grid with `spacing` mm by the rule above; `mode` softmax or sigmoid, `thresh` the logit a sigmoid
    decision is taken at.  A grid no axis of which is linked is refused naming the subject and the spacing."""
    r = linked_radii(sn, spacing, params)
    step = step or ops_crf.seg_crf
    out, changed = step(ops, logits, images, tuple(float(s) for s in spacing), mode, *params, thresh)
    return out, changed, r
