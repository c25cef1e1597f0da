"""The device halves of the rigid registration (effq_prep_bins, effq_prep_joint_hist; the rule of register.py and of
prep.py's --prep_register): free functions over a HipOps, as ops_align.prep_align is, which keeps the surface of HipOps
and of its mixins what it is."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr

BINS, SKIP, MAX_K = _lib.PREP_REGISTER_BINS, _lib.PREP_REGISTER_SKIP, _lib.PREP_REGISTER_MAX_K


def _volume(ops, what: str, x, dtype):
    """The checked extents of a contiguous D x H x W device tensor of `dtype`."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != dtype or x.numel() == 0 or not x.is_contiguous() \
            or ops._elsewhere(x):
        raise _lib.EffqError(f"{what}: needs a contiguous D x H x W {dtype} tensor on {ops.device}, got "
                             f"{tuple(getattr(x, 'shape', ()))} {getattr(x, 'dtype', type(x))} on "
                             f"{getattr(x, 'device', None)}")
    dims = tuple(int(n) for n in x.shape)
    if max(dims) > 32767 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise _lib.EffqError(f"{what}: extents {dims}: three of 1 ... 32767, 2^31 - 1 voxels in all at most")
    return dims


def _bin_range(what: str, lo, scale):
    lo, scale = float(np.float32(lo)), float(np.float32(scale))
    if not (math.isfinite(lo) and math.isfinite(scale) and scale > 0.0):
        raise _lib.EffqError(f"{what}: bin range lo {lo}, scale {scale}: needs finite values and a scale above 0")
    return lo, scale


def prep_bins(ops, x: torch.Tensor, lo: float, scale: float, mask_nonzero: bool = False) -> torch.Tensor:
    """The D x H x W float32 volume `x` as one uint8 per voxel: its bin min(max(int((x - lo) * scale), 0), BINS - 1) in
    fp32, or SKIP (255, "not sampled") for a NaN and, with `mask_nonzero`, for a voxel that is exactly 0.  A new tensor."""
    what = "prep_bins"
    dims = _volume(ops, what, x, torch.float32)
    lo, scale = _bin_range(what, lo, scale)
    y = torch.empty(dims, dtype=torch.uint8, device=ops.device)
    check(ops.lib.effq_prep_bins(_ptr(x), dims[0], dims[1], dims[2], lo, scale, int(bool(mask_nonzero)), _ptr(y),
                                 ops.stream), "effq_prep_bins")
    return y


def prep_joint_hist(ops, fbin: torch.Tensor, mov: torch.Tensor, matrices, lo: float, scale: float,
                    stride=(1, 1, 1)) -> torch.Tensor:
    """The joint histograms of the reference's bins `fbin` (D x H x W uint8, prep_bins) and the bins of the float32
    volume `mov` sampled trilinearly through each of the K candidate `matrices` (K x 3 x 4, fp64, host; each maps a
    reference voxel index to voxel coordinates of `mov`, prep.align_matrix), over the reference voxels at the sample
    `stride` (sd, sh, sw).  `lo`, `scale`: the bin range of `mov`.  Returns int64 [K, BINS, BINS] on the device:
    [k, bf, bm] counts the sampled voxels with reference bin bf whose sample under matrix k lies inside the field of view
    of `mov`, is not NaN and has bin bm."""
    what = "prep_joint_hist"
    dims, mdims = _volume(ops, what, fbin, torch.uint8), _volume(ops, what, mov, torch.float32)
    try:
        m = np.ascontiguousarray(np.asarray(matrices, dtype=np.float64).reshape(-1, 12))
        s = tuple(int(v) for v in stride)
    except (TypeError, ValueError) as e:
        raise _lib.EffqError(f"{what}: matrices or stride: {e}") from e
    if not 1 <= m.shape[0] <= MAX_K:
        raise _lib.EffqError(f"{what}: {m.shape[0]} matrices, needs 1 ... {MAX_K}")
    if not np.all(np.isfinite(m)):
        raise _lib.EffqError(f"{what}: a matrix holds an entry that is not finite")
    if len(s) != 3 or min(s) < 1:
        raise _lib.EffqError(f"{what}: stride {s}: three integers >= 1")
    lo, scale = _bin_range(what, lo, scale)
    hist = torch.empty((m.shape[0], BINS, BINS), dtype=torch.int64, device=ops.device)
    # the matrices are a host array, read before the call returns
    check(ops.lib.effq_prep_joint_hist(_ptr(fbin), dims[0], dims[1], dims[2], _ptr(mov), mdims[0], mdims[1], mdims[2],
                                       m.ctypes.data, m.shape[0], lo, scale, s[0], s[1], s[2], _ptr(hist), ops.stream),
          "effq_prep_joint_hist")
    return hist
