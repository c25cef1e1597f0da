"""The device steps of the non-local means denoiser (effq_prep_denoise_residual, effq_prep_denoise_nlm; the rule of
denoise.py and of prep.py's --prep_denoise): free functions over a HipOps, as those of ops_bias are."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr
from .ops_register import _volume

TILE, MAX_RADIUS = _lib.PREP_DENOISE_TILE, _lib.PREP_DENOISE_MAX_RADIUS


def _mask(what: str, mask: str) -> int:
    if mask not in _lib.PREP_MASKS:
        raise _lib.EffqError(f"{what}: mask {mask!r}, one of {', '.join(_lib.PREP_MASKS)}")
    return _lib.PREP_MASKS[mask]


def prep_denoise_residual(ops, v: torch.Tensor, mask: str = "nonzero") -> torch.Tensor:
    """r of the D x H x W float32 scan `v`: |v - the mean of its six face neighbours| (fp64, rounded once) where the voxel
    and the six are inside the volume, finite and in `mask`; +0 everywhere else.  A new tensor."""
    what = "prep_denoise_residual"
    dims = _volume(ops, what, v, torch.float32)
    mode = _mask(what, mask)
    r = torch.empty_like(v)
    check(ops.lib.effq_prep_denoise_residual(_ptr(v), *dims, mode, _ptr(r), ops.stream), "effq_prep_denoise_residual")
    return r


def prep_denoise_nlm(ops, v: torch.Tensor, mask: str, radius: int, sigma: float):
    """(y, sumsq, count): y the non-local means of `v` at search radius `radius` (1 ... MAX_RADIUS) and noise level
    `sigma`, a new tensor; sumsq the fp64 sum of (y - v)^2 over the finite voxels of `mask` and count their number, host
    values: the call reads them back."""
    what = "prep_denoise_nlm"
    dims = _volume(ops, what, v, torch.float32)
    mode = _mask(what, mask)
    if not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise _lib.EffqError(f"{what}: search radius {radius!r}, needs 1 ... {MAX_RADIUS}")
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0 and math.isfinite(sigma * sigma) and sigma * sigma > 0.0):
        raise _lib.EffqError(f"{what}: sigma {sigma!r}, needs a finite value above 0")
    need = C.c_size_t()
    check(ops.lib.effq_prep_denoise_ws_bytes(*dims, C.byref(need)), "effq_prep_denoise_ws_bytes")
    ws = ops._workspace("prep_denoise", need.value)
    y = torch.empty_like(v)
    change = torch.empty(2, dtype=torch.float64, device=ops.device)
    check(ops.lib.effq_prep_denoise_nlm(_ptr(v), *dims, mode, radius, sigma * sigma, _ptr(y), _ptr(change), _ptr(ws),
                                        ws.numel(), ops.stream), "effq_prep_denoise_nlm")
    sumsq, count = change.cpu().tolist()
    return y, sumsq, int(count)
