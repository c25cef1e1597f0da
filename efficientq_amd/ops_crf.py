"""The device step of the local conditional random field (effq_seg_crf; the rule of crf.py and of predict's --crf): a
free function over a HipOps, as those of ops_denoise are."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr

TILE, MAX_RADIUS = _lib.SEG_CRF_TILE, _lib.SEG_CRF_MAX_RADIUS
MODES = {"softmax": _lib.SEG_ARGMAX, "sigmoid": _lib.SEG_SIGMOID}


def _planes(ops, what: str, name: str, x, most: int):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32 or x.numel() == 0 or \
            not x.is_contiguous() or ops._elsewhere(x) or x.shape[0] > most:
        raise _lib.EffqError(f"{what}: {name} needs a contiguous (1 ... {most}) x D x H x W float32 tensor on {ops.device}, "
                             f"got {tuple(getattr(x, 'shape', ()))} {getattr(x, 'dtype', type(x))} on "
                             f"{getattr(x, 'device', None)}")
    return tuple(int(n) for n in x.shape)


def seg_crf(ops, logits: torch.Tensor, images: torch.Tensor, spacing, mode: str, w_a: float, w_s: float, theta_p: float,
            theta_i: float, theta_s: float, iters: int, thresh: float = 0.0):
    """(H, changed): the (C, D, H, W) float32 `logits` after `iters` mean-field iterations of the rule of crf.py, a new
    tensor, with the pair weights from the (M, D, H, W) float32 `images` of the same grid at `spacing` (d, h, w in mm);
    `mode` softmax (class ids) or sigmoid (every channel a binary field, decided at the logit `thresh`).  changed, a host
    value the call reads back: the voxels whose decision differs between `logits` and H.  What the entry point refuses
    (include/effq_hip.h) raises EffqError."""
    what = "seg_crf"
    if mode not in MODES:
        raise _lib.EffqError(f"{what}: mode {mode!r}, one of {', '.join(MODES)}")
    shape = _planes(ops, what, "logits", logits, _lib.SEG_CRF_MAX_CLASSES)
    if _planes(ops, what, "images", images, _lib.SEG_CRF_MAX_MODALITIES)[1:] != shape[1:]:
        raise _lib.EffqError(f"{what}: logits {shape} and images {tuple(images.shape)} are not on one grid")
    if len(tuple(spacing)) != 3:
        raise _lib.EffqError(f"{what}: spacing {spacing!r}, needs d, h, w in mm")
    need = C.c_size_t()
    check(ops.lib.effq_seg_crf_ws_bytes(*shape, C.byref(need)), "effq_seg_crf_ws_bytes")
    ws = ops._workspace("seg_crf", need.value)
    out = torch.empty_like(logits)
    changed = torch.empty(1, dtype=torch.int32, device=ops.device)
    check(ops.lib.effq_seg_crf(_ptr(logits), shape[0], _ptr(images), int(images.shape[0]), *shape[1:],
                               *(float(s) for s in spacing), MODES[mode], float(w_a), float(w_s), float(theta_p),
                               float(theta_i), float(theta_s), int(iters), float(thresh), _ptr(out), _ptr(changed), _ptr(ws),
                               ws.numel(), ops.stream), "effq_seg_crf")
    return out, int(changed.cpu()[0])
