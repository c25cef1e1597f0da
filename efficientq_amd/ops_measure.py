"""One geometric record per lesion of finished label maps (effq_label_lesion_measures): a free function over a HipOps,
as ops_score's, which keeps the surface of HipOps and of its mixins what it is."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr
from .ops_score import _maps

SLICE_AXES = (0, 1, 2)


def label_lesion_measures(ops, pred: torch.Tensor, truth, lut, C_: int, spacing, slice_axis: int,
                          connectivity: int = _lib.LESION_CONNECTIVITY, max_rows=None):
    """The lesions of a uint8 label map `pred` and, when `truth` is not None, of the label map `truth` of the same
    D x H x W grid, one by one (effq_label_lesion_measures).  `lut` and `C_` as ops_score.label_lesions, `spacing`
    (d, h, w) in mm as ops.seg_surface_mm, `slice_axis` the array axis the slices are stacked along.  Returns (counts,
    nrows, rows, meas) on the host: counts C x 4 int64, bit for bit label_lesions' (None without `truth`); nrows (P)
    int64, the components of plane q - the predicted mask of class q for q < C, the label mask of class q - C after
    them (P = 2 C with `truth`, C without); rows, a list of P int32 tensors n_q x 3 = first voxel (linear index), size,
    overlap, in ascending order of the first voxel; meas, a list of P int64 tensors n_q x _lib.LESION_MEASURE_WORDS =
    the sums of d, h, w, the box (min d, h, w, max d, h, w), the end points a <= b of the 3-D diameter and those of the
    diameter inside one slice (linear indices).  max_rows: the rows per plane asked for first (default
    _lib.LESION_TABLE_ROWS); a plane with more components costs one more call, all rows are returned.  A call whose
    components have more than _lib.LESION_MEASURE_MAX_TILE_PAIRS tile pairs in all is not searched and raises."""
    what = "label_lesion_measures"
    p, t, table, Cc, (D, H, W) = _maps(ops, what, pred, pred if truth is None else truth, lut, C_)
    if connectivity not in (6, 26):
        raise _lib.EffqError(f"{what}: connectivity {connectivity!r}, 6 or 26")
    if slice_axis not in SLICE_AXES:
        raise _lib.EffqError(f"{what}: slice_axis {slice_axis!r}, one of 0, 1, 2")
    wd, wh, ww = ops._axis_weights(what, spacing)
    P = Cc if truth is None else 2 * Cc
    if P * D * H * W >= 2 ** 31 or max(D, H, W) > _lib.EDT_MM_MAX_EXTENT:
        raise _lib.EffqError(f"{what}: {P} masks of {D} x {H} x {W} voxels (2^31 - 1 voxels in all at most, every extent "
                             f"at most {_lib.EDT_MM_MAX_EXTENT})")
    cap = _lib.LESION_TABLE_ROWS if max_rows is None else int(max_rows)
    if cap <= 0:
        raise _lib.EffqError(f"{what}: max_rows {max_rows}, needs a positive capacity")
    words = _lib.LESION_MEASURE_WORDS
    while True:
        need = ops.lib.effq_label_lesion_measures_ws_bytes(Cc, P, D, H, W, cap)
        if need == 0:
            raise _lib.EffqError(f"{what}: a table of {P} x {cap} rows")
        counts = None if truth is None else torch.empty(Cc, 4, dtype=torch.int64, device=ops.device)
        nrows = torch.empty(P, dtype=torch.int64, device=ops.device)
        rows = torch.empty(P, cap, 3, dtype=torch.int32, device=ops.device)
        meas = torch.empty(P, cap, words, dtype=torch.int64, device=ops.device)
        ws = ops._workspace("lesion_measures", need)
        check(ops.lib.effq_label_lesion_measures(
            _ptr(p), None if truth is None else _ptr(t), Cc, D, H, W, table, int(connectivity), wd, wh, ww,
            int(slice_axis), cap, None if counts is None else _ptr(counts), _ptr(nrows), _ptr(rows), _ptr(meas), _ptr(ws),
            ws.numel(), ops.stream), "effq_label_lesion_measures")
        nrows = nrows.cpu()
        most = int(nrows.max())
        if most <= cap:
            rows, meas = rows[:, :most].cpu(), meas[:, :most].cpu()
            n = [int(v) for v in nrows]
            if any(n[q] and int(meas[q, 0, 9]) < 0 for q in range(P)):
                raise _lib.EffqError(f"{what}: the components of these maps have more than "
                                     f"{_lib.LESION_MEASURE_MAX_TILE_PAIRS} pairs of tiles of 256 line ends in all (the "
                                     f"search grows with the square of the line ends of a component; a map of noise that "
                                     f"hangs together is the case): the diameters were not searched")
            return (None if counts is None else counts.cpu(), nrows, [rows[q, :n[q]] for q in range(P)],
                    [meas[q, :n[q]] for q in range(P)])
        cap = most
