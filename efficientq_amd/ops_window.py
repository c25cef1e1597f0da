"""The sliding window of the validation on whole volumes (evaluate.validate_seg): window grid, gather, put, stitch
and the blend weights (effq_window_*)."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops_base import OpsBase, _ptr, _triple


def _flip_mask(flip, who: str) -> int:
    if isinstance(flip, bool) or int(flip) != flip or not 0 <= flip <= 7:
        raise _lib.EffqError(f"{who}: flip mask {flip!r}, an int 0..7 (bit 0 = d, bit 1 = h, bit 2 = w)")
    return int(flip)


BLEND_KINDS = ("uniform", "gauss")


def blend_weights_host(patch, kind: str = "uniform"):
    """The per-axis window weights of the blend `kind` for the window extent `patch`, three fp32 numpy vectors whose
    outer product weighs a window's voxels.  uniform: ones.  gauss: w(i) = exp(-0.5 ((i - (p - 1) / 2) / (p / 8))^2),
    sigma = patch / 8 with the peak 1 at the centre, computed in fp64 and rounded once to fp32.  The least value of an
    axis is exp(-0.5 (4 (p - 1) / p)^2) > exp(-8) = 3.4e-4 at any p, so the least product of three is above 3.7e-11:
    thirty orders of magnitude from the fp32 denormals, and no floor is needed."""
    if kind not in BLEND_KINDS:
        raise _lib.EffqError(f"blend {kind!r}, one of {', '.join(BLEND_KINDS)}")
    out = []
    for p in _triple(patch):
        if p <= 0:
            raise _lib.EffqError(f"window extent {p} must be positive")
        if kind == "uniform":
            out.append(np.ones(p, dtype=np.float32))
        else:
            i = np.arange(p, dtype=np.float64)
            out.append(np.exp(-0.5 * ((i - (p - 1) / 2.0) / (p / 8.0)) ** 2).astype(np.float32))
    return tuple(out)


class WindowOps(OpsBase):
    """The window wrappers of HipOps."""

    @staticmethod
    def window_grid(dhw, patch, overlap) -> Tuple[int, int, int]:
        """Windows per axis of evaluate.window_starts; raises on a window larger than the volume or an overlap that
        is not smaller than the window."""
        n = []
        for s, p, o in zip(dhw, _triple(patch), _triple(overlap)):
            if p <= 0 or p > s:
                raise _lib.EffqError(f"window extent {p} outside 1..{s}")
            if o < 0 or o >= p:
                raise _lib.EffqError(f"overlap {o} must lie in 0..{p - 1}")
            n.append(len(range(0, s - p, p - o)) + 1)
        return tuple(n)

    def _window_case(self, shape, patch, overlap):
        """(N, C, D, H, W, patch, overlap, number of windows) of the N x C x D x H x W volume `shape`, window_grid's
        refusals applied."""
        N, Cc, D, H, W = (int(i) for i in shape)
        p, o = _triple(patch), _triple(overlap)
        return N, Cc, D, H, W, p, o, math.prod(self.window_grid((D, H, W), p, o))

    @staticmethod
    def _window_channels(what: str, Cc: int):
        if not 0 < Cc <= 8:
            raise _lib.EffqError(f"{what}: {Cc} channels, at most 8")

    def window_gather(self, vol: torch.Tensor, patch, overlap, first: int = 0, count: Optional[int] = None,
                      flip: int = 0):
        """Windows first .. first+count-1 of the N x C x D x H x W volume as one (count*N, pd, ph, pw, C)
        channels-last batch, window-major, the content of every window mirrored along the axes of the mask `flip`
        (bit 0 = d, bit 1 = h, bit 2 = w; effq_window_gather)."""
        x = self._f32(vol)
        if x.dim() != 5:
            raise _lib.EffqError(f"window_gather: expected N x C x D x H x W, got {tuple(x.shape)}")
        flip = _flip_mask(flip, "window_gather")
        N, Cc, D, H, W, p, o, nwin = self._window_case(x.shape, patch, overlap)
        count = nwin - first if count is None else int(count)
        if first < 0 or count <= 0 or first + count > nwin:
            raise _lib.EffqError(f"windows {first}..{first + count - 1} of {nwin}")
        out = torch.empty(count * N, p[0], p[1], p[2], Cc, dtype=torch.float32, device=self.device)
        check(self.lib.effq_window_gather(_ptr(x), N, Cc, D, H, W, p[0], p[1], p[2], o[0], o[1], o[2], int(first), count,
                                          flip, _ptr(out), self.stream), "effq_window_gather")
        return out

    def window_put(self, last: torch.Tensor, buf_slice: torch.Tensor, flip: int = 0, accumulate: bool = False) -> None:
        """A network's last head `last` (M x C x pd x ph x pw, the windows of one batch mirrored by `flip`) into
        `buf_slice`, the M x pd x ph x pw x C slice of the stitch's window buffer: transposed to channels-last,
        un-mirrored, and stored (accumulate=False) or added onto what the slice holds (effq_window_put).  The slice is
        written in place: it must be fp32, contiguous and on this device.  A head with channels-last strides (from_ndhwc:
        what the convs of this package return) stored with flip 0 is in the slice's layout already, and the bits are
        copied device to device as they lie; for any other pass such a head is first made contiguous, which allocates
        a tensor of its size."""
        if last.dim() != 5:
            raise _lib.EffqError(f"window_put: expected M x C x pd x ph x pw, got {tuple(last.shape)}")
        flip = _flip_mask(flip, "window_put")
        M, Cc, pd, ph, pw = (int(i) for i in last.shape)
        self._window_channels("window_put", Cc)
        if tuple(buf_slice.shape) != (M, pd, ph, pw, Cc):
            raise _lib.EffqError(f"window_put: buffer slice {tuple(buf_slice.shape)}, the head needs {(M, pd, ph, pw, Cc)}")
        if self._f32(buf_slice) is not buf_slice:
            raise _lib.EffqError("window_put: the buffer slice is written in place and must be contiguous")
        if M * Cc * pd * ph * pw >= 1 << 31:
            raise _lib.EffqError(f"window_put: {M * Cc * pd * ph * pw} elements, fewer than 2^31 per call")
        as_stored = last.permute(0, 2, 3, 4, 1)
        if flip == 0 and not accumulate and not last.is_contiguous() and as_stored.is_contiguous():
            buf_slice.copy_(self._f32(as_stored))           # _f32: the checks of device and dtype, no copy
            return
        src = self._f32(last)
        check(self.lib.effq_window_put(_ptr(src), M, Cc, pd, ph, pw, flip, int(bool(accumulate)), _ptr(buf_slice),
                                       self.stream), "effq_window_put")

    def window_stitch(self, win: torch.Tensor, shape, patch, overlap, weights=None, nflip: int = 1) -> torch.Tensor:
        """The window buffer, (nwin*N, pd, ph, pw, C) channels-last and window-major and holding the sum of `nflip`
        passes, stitched to the N x C x D x H x W volume `shape` (effq_window_stitch).  weights=None: each voxel is the
        sum over its covering windows over (nflip * their count); with nflip = 1 evaluate.patch_to_image3d.  Otherwise
        the separable per-axis `weights` (three fp32 device tensors of pd, ph, pw values: blend_weights): the weighted
        sum over (nflip * the sum of the weights).  Ones give the bits of None."""
        w = self._f32(win)
        N, Cc, D, H, W, p, o, nwin = self._window_case(shape, patch, overlap)
        if tuple(w.shape) != (nwin * N, p[0], p[1], p[2], Cc):
            raise _lib.EffqError(f"window_stitch: windows {tuple(w.shape)}, geometry needs {(nwin * N, *p, Cc)}")
        self._window_channels("window_stitch", Cc)
        if int(nflip) != nflip or nflip < 1:
            raise _lib.EffqError(f"window_stitch: nflip {nflip!r}, the number of passes summed, is at least 1")
        ws = (None, None, None)
        if weights is not None:
            if len(weights) != 3:
                raise _lib.EffqError(f"window_stitch: {len(weights)} weight tensors, one per axis d, h, w")
            ws = [self._f32(t) for t in weights]
            for t, n, ax in zip(ws, p, "dhw"):
                if t.dim() != 1 or int(t.numel()) != n:
                    raise _lib.EffqError(f"window_stitch: weights of axis {ax} have shape {tuple(t.shape)}, the window "
                                         f"needs ({n},)")
        out = torch.empty(N, Cc, D, H, W, dtype=torch.float32, device=self.device)
        check(self.lib.effq_window_stitch(_ptr(w), N, Cc, D, H, W, p[0], p[1], p[2], o[0], o[1], o[2], _ptr(ws[0]),
                                          _ptr(ws[1]), _ptr(ws[2]), int(nflip), _ptr(out), self.stream),
              "effq_window_stitch")
        return out

    def blend_weights(self, patch, kind: str = "uniform"):
        """The three per-axis fp32 weight tensors of window_stitch on this device (blend_weights_host)."""
        return tuple(torch.from_numpy(w).to(self.device) for w in blend_weights_host(patch, kind))
