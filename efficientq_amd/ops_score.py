"""Scoring a finished label map against a label map on one grid (effq_label_lesions, effq_label_surface_mm): free
functions over a HipOps, which keeps the surface of HipOps and of its mixins what it is.  The Dice tallies of the same
two maps are ``ops.label_tallies``."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr


def tolerances_sq(what: str, tols):
    """The fp32 squared tolerances float32(float64(tol_mm) ** 2) of `tols` (millimetres), as the axis weights are
    computed: at most _lib.SURF_TOL_MAX, each finite and >= 0, strictly ascending (also after the rounding)."""
    try:
        t = [float(v) for v in tols]
    except (TypeError, ValueError) as e:
        raise _lib.EffqError(f"{what}: tols {tols!r}: {e}") from e
    if len(t) > _lib.SURF_TOL_MAX:
        raise _lib.EffqError(f"{what}: tols: {len(t)} tolerances, at most {_lib.SURF_TOL_MAX}")
    if not all(math.isfinite(v) and v >= 0 for v in t):
        raise _lib.EffqError(f"{what}: tols {t}: every tolerance is finite and >= 0 (millimetres)")
    with np.errstate(over="ignore"):
        sq = [float(np.float32(np.float64(v) ** 2)) for v in t]
    if not all(math.isfinite(v) for v in sq) or any(b <= a for a, b in zip(sq, sq[1:])):
        raise _lib.EffqError(f"{what}: tols {t}: the squares must be finite in fp32 and strictly ascending")
    return sq


def _maps(ops, what: str, pred: torch.Tensor, truth: torch.Tensor, lut, C_: int):
    """(pred, truth, table, C, (D, H, W)) of the two maps of one case, checked: D x H x W uint8 of one shape on the device
    of `ops`, contiguous copies where needed; 256 table entries of C class bits each."""
    Cc = int(C_)
    for t, who in ((pred, "pred"), (truth, "truth")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.numel() == 0:
            raise _lib.EffqError(f"{what}: {who} {tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}: needs a "
                                 f"D x H x W torch.uint8 label map, not empty")
        if ops._elsewhere(t):
            raise _lib.EffqError(f"{what}: {who} on {t.device}, ops on {ops.device}")
    if tuple(truth.shape) != tuple(pred.shape):
        raise _lib.EffqError(f"{what}: truth {tuple(truth.shape)} for a map {tuple(pred.shape)}: needs the map's shape")
    if not 0 < Cc <= _lib.SEG_TALLIES_MAX_CLASSES:
        raise _lib.EffqError(f"{what}: {Cc} classes, at most {_lib.SEG_TALLIES_MAX_CLASSES}")
    try:
        table = [int(v) for v in lut]
    except (TypeError, ValueError) as e:
        raise _lib.EffqError(f"{what}: lut: {e}") from e
    if len(table) != 256 or min(table) < 0 or max(table) >= 1 << Cc:
        raise _lib.EffqError(f"{what}: lut of {len(table)} entries, needs 256 of {Cc} class bits each")
    return pred.contiguous(), truth.contiguous(), (C.c_uint16 * 256)(*table), Cc, tuple(int(e) for e in pred.shape)


def label_lesions(ops, pred: torch.Tensor, truth: torch.Tensor, lut, C_: int,
                  connectivity: int = _lib.LESION_CONNECTIVITY) -> torch.Tensor:
    """The lesion-level columns (C x 4 int64 on the device: totall, predl, fnl, fpl, as ops.seg_lesions) of a uint8 label
    map `pred` against the label map `truth` of the same D x H x W grid (effq_label_lesions).  `lut` as
    ops.label_tallies: 256 integers, bit c set = that label value belongs to class c."""
    what = "label_lesions"
    p, t, table, Cc, (D, H, W) = _maps(ops, what, pred, truth, lut, C_)
    if connectivity not in (6, 26):
        raise _lib.EffqError(f"{what}: connectivity {connectivity!r}, 6 or 26")
    if 2 * Cc * D * H * W >= 2 ** 31:
        raise _lib.EffqError(f"{what}: {2 * Cc} masks of {D * H * W} voxels (2^31 - 1 voxels in all at most)")
    counts = torch.empty(Cc, 4, dtype=torch.int64, device=ops.device)
    ws = ops._workspace("cc", ops.lib.effq_cc_ws_bytes(2 * Cc, D, H, W))
    check(ops.lib.effq_label_lesions(_ptr(p), _ptr(t), Cc, D, H, W, table, int(connectivity), _ptr(counts), _ptr(ws),
                                     ws.numel(), ops.stream), "effq_label_lesions")
    return counts


def label_surface_mm(ops, pred: torch.Tensor, truth: torch.Tensor, lut, C_: int, spacing, tols=()):
    """What the surface distances in millimetres and the normalised surface Dice of a uint8 label map `pred` against the
    label map `truth` need (effq_label_surface_mm); maps and `lut` as label_lesions, `spacing` (d, h, w) in mm as
    ops.seg_surface_mm.  Returns (counts, sq, sums, within) on the device: the first three are ops.seg_surface_mm's
    (evaluate.surface_metrics_mm turns them into hd, hd95 and assd); within C x 2 x len(tols) int64 = the voxels of S(P)
    within `tols[k]` mm of S(L), and those of S(L) within it of S(P) (a surface whose target is empty has none), with
    the comparison E <= float32(float64(tol) ** 2) in fp32.  `tols`: at most _lib.SURF_TOL_MAX, ascending."""
    what = "label_surface_mm"
    p, t, table, Cc, (D, H, W) = _maps(ops, what, pred, truth, lut, C_)
    wd, wh, ww = ops._axis_weights(what, spacing)
    sqt = tolerances_sq(what, tols)
    need = ops.lib.effq_label_surface_mm_ws_bytes(Cc, D, H, W, len(sqt))
    if need == 0:
        raise _lib.EffqError(f"{what}: {2 * Cc} masks of {D} x {H} x {W} voxels (2^31 - 1 voxels in all at most, every "
                             f"extent at most {_lib.EDT_MM_MAX_EXTENT})")
    counts = torch.empty(Cc, 2, dtype=torch.int64, device=ops.device)
    sq = torch.empty(Cc, 4, dtype=torch.float32, device=ops.device)
    sums = torch.empty(Cc, 2, dtype=torch.float64, device=ops.device)
    within = torch.empty(Cc, 2, len(sqt), dtype=torch.int64, device=ops.device)
    ws = ops._workspace("surf_mm", need)
    check(ops.lib.effq_label_surface_mm(_ptr(p), _ptr(t), Cc, D, H, W, table, wd, wh, ww, (C.c_float * len(sqt))(*sqt),
                                        len(sqt), _ptr(counts), _ptr(sq), _ptr(sums), _ptr(within) if sqt else None,
                                        _ptr(ws), ws.numel(), ops.stream), "effq_label_surface_mm")
    return counts, sq, sums, within
