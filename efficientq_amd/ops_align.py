"""Resampling one volume onto another grid through a general affine (effq_prep_align; the rule of prep.py's
--prep_align): a free function over a HipOps, which keeps the surface of HipOps and of its mixins what it is."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr


def prep_align(ops, x: torch.Tensor, matrix, out_shape, nearest: bool = False):
    """The D x H x W volume `x` on the grid of `out_shape` (OD, OH, OW): `matrix` (3 x 4, fp64, host) maps an output voxel
    index (d, h, w, 1) to voxel coordinates of `x` (prep.align_matrix).  A float32 volume is interpolated trilinearly,
    with `nearest` the volume is a uint8 label and keeps its values; outside the field of view of `x` the result is 0.
    Returns (y, inside): a new tensor on the device, and a one-element int64 device tensor, the number of voxels of `y`
    that lie inside the field of view."""
    what = "prep_align"
    dtype = torch.uint8 if nearest else torch.float32
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != dtype or x.numel() == 0 or not x.is_contiguous() \
            or ops._elsewhere(x):
        raise _lib.EffqError(f"{what}: needs a contiguous D x H x W {dtype} tensor on {ops.device}, got "
                             f"{tuple(getattr(x, 'shape', ()))} {getattr(x, 'dtype', type(x))} on "
                             f"{getattr(x, 'device', None)}")
    try:
        m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64).reshape(12))
        o = tuple(int(v) for v in out_shape)
    except (TypeError, ValueError) as e:
        raise _lib.EffqError(f"{what}: matrix or out_shape: {e}") from e
    if not np.all(np.isfinite(m)):
        raise _lib.EffqError(f"{what}: the matrix holds an entry that is not finite")
    dims = tuple(int(n) for n in x.shape)
    for shape in (dims, o):
        if len(shape) != 3 or min(shape) < 1 or max(shape) > 32767 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
            raise _lib.EffqError(f"{what}: extents {shape}: three of 1 ... 32767, 2^31 - 1 voxels in all at most")
    y = torch.empty(o, dtype=dtype, device=ops.device)
    inside = torch.empty(1, dtype=torch.int64, device=ops.device)
    # the matrix is a host array, read before the call returns
    check(ops.lib.effq_prep_align(_ptr(x), dims[0], dims[1], dims[2], m.ctypes.data,
                                  _lib.PREP_NEAREST if nearest else _lib.PREP_LINEAR, _ptr(y), o[0], o[1], o[2],
                                  _ptr(inside), ops.stream), "effq_prep_align")
    return y, inside
