"""The prep mission (prep.py): windows and percentiles, resampling, smoothing, moments, standardising, cropping and
reorientation of source scans (effq_prep_*)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops_base import OpsBase, _ptr


def _flat_f32(ops: "PrepOps", what: str, x: torch.Tensor, lo, hi, mask: Optional[str] = None) -> Optional[int]:
    """The checks of prep_window and prep_window_mask: `x` a contiguous float32 tensor on the device of `ops`, not empty,
    and lo <= hi.  With `mask`: its code, refused between the two as prep_window_mask always did."""
    if x.dtype != torch.float32 or not x.is_contiguous() or ops._elsewhere(x) or x.numel() == 0:
        raise _lib.EffqError(f"{what}: needs a contiguous float32 tensor on {ops.device}")
    mode = None if mask is None else ops._prep_mask(what, mask)
    if not float(lo) <= float(hi):
        raise _lib.EffqError(f"{what}: bounds {lo}, {hi}")
    return mode


def _resample_geometry(what: str, factors, out_shape, N: int):
    """(factors, output extents) of prep_resample and prep_resample_cubic as tuples of three, bounded for N volumes."""
    f = tuple(float(v) for v in factors)
    o = tuple(int(v) for v in out_shape)
    if len(f) != 3 or len(o) != 3 or not all(0.0 < v <= 1e6 for v in f) or min(o) < 1 or max(o) > 32767 or \
            N * o[0] * o[1] * o[2] >= 2 ** 31:
        raise _lib.EffqError(f"{what}: factors {f}, output extents {o}")
    return f, o


class PrepOps(OpsBase):
    """The prep wrappers of HipOps."""

    def _prep_volumes(self, what: str, x: torch.Tensor, dtype=torch.float32, limit_c: bool = True):
        """The checked (tensor, C, D, H, W) of a contiguous C x D x H x W device tensor of `dtype`."""
        if x.dim() != 4 or x.dtype != dtype or x.numel() == 0 or not x.is_contiguous() or self._elsewhere(x):
            raise _lib.EffqError(f"{what}: needs a contiguous C x D x H x W {dtype} tensor on {self.device}, got "
                                 f"{tuple(x.shape)} {x.dtype} on {x.device}")
        Cc, D, H, W = (int(n) for n in x.shape)
        if (limit_c and Cc > _lib.PREP_MAX_MODALITIES) or x.numel() >= 2 ** 31 or max(D, H, W) > 32767:
            raise _lib.EffqError(f"{what}: shape {tuple(x.shape)}: at most {_lib.PREP_MAX_MODALITIES} modalities, 2^31 - 1 "
                                 f"voxels in all and 32767 along an axis")
        return x, Cc, D, H, W

    @staticmethod
    def _prep_mask(what: str, mask: str) -> int:
        if mask not in _lib.PREP_MASKS:
            raise _lib.EffqError(f"{what}: unknown mask {mask!r} (one of {', '.join(_lib.PREP_MASKS)})")
        return _lib.PREP_MASKS[mask]

    @staticmethod
    def _prep_box(what: str, shape, pmin, pmax):
        lo, hi = tuple(int(v) for v in pmin), tuple(int(v) for v in pmax)
        if len(lo) != 3 or len(hi) != 3 or not all(0 <= a < b <= n for a, b, n in zip(lo, hi, shape)):
            raise _lib.EffqError(f"{what}: box {lo} : {hi} does not lie in a grid of {tuple(shape)}")
        return lo, hi, (C.c_int * 3)(*lo), (C.c_int * 3)(*hi)

    def _prep_stats(self, what: str, v, n: int) -> torch.Tensor:
        t = torch.as_tensor(v, dtype=torch.float64).reshape(-1).to(self.device)
        if t.numel() != n:
            raise _lib.EffqError(f"{what}: {t.numel()} values for {n} modalities")
        return t

    def prep_window(self, x: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
        """Clip the float32 tensor `x` to [lo, hi] in place (effq_prep_window: numpy.clip, a NaN stays)."""
        _flat_f32(self, "prep_window", x, lo, hi)
        check(self.lib.effq_prep_window(_ptr(x), x.numel(), float(lo), float(hi), self.stream), "effq_prep_window")
        return x

    def prep_quantiles(self, x: torch.Tensor, qs, mask: str = "nonzero"):
        """The order statistics around the percentiles `qs` (1 to PREP_QUANTILE_MAX values in [0, 100]) of every
        modality of x = C x S (or C x D x H x W) float32 over its own mask (effq_prep_quantiles; the rule of prep.py's
        --prep_window pLO,pHI).  Returns (count int64[C], stats float32[C, len(qs), 2]) on the device: stats[c, r] =
        sorted[k], sorted[min(k + 1, n - 1)] with k = floor((n - 1) qs[r] / 100); NaN where the mask is empty.
        prep.percentile_value interpolates between the two."""
        if x.dim() < 2 or x.dtype != torch.float32 or x.numel() == 0 or not x.is_contiguous() or self._elsewhere(x):
            raise _lib.EffqError(f"prep_quantiles: needs a contiguous C x S float32 tensor on {self.device}, got "
                                 f"{tuple(x.shape)} {x.dtype} on {x.device}")
        Cc = int(x.shape[0])
        if Cc > _lib.PREP_MAX_MODALITIES or x.numel() >= 2 ** 31:
            raise _lib.EffqError(f"prep_quantiles: shape {tuple(x.shape)}: at most {_lib.PREP_MAX_MODALITIES} modalities and "
                                 f"2^31 - 1 voxels in all")
        mode = self._prep_mask("prep_quantiles", mask)
        try:
            q = [float(v) for v in qs]
        except (TypeError, ValueError):
            q = []
        if not 1 <= len(q) <= _lib.PREP_QUANTILE_MAX or not all(0.0 <= v <= 100.0 for v in q):
            raise _lib.EffqError(f"prep_quantiles: percentiles {qs!r}: needs 1 to {_lib.PREP_QUANTILE_MAX} values in "
                                 f"[0, 100]")
        count = torch.empty(Cc, dtype=torch.int64, device=self.device)
        stats = torch.empty((Cc, len(q), 2), dtype=torch.float32, device=self.device)
        need = C.c_size_t()
        check(self.lib.effq_prep_quantile_ws_bytes(C.byref(need)), "effq_prep_quantile_ws_bytes")
        ws = self._workspace("prep_quantile", need.value)
        # the percentiles are host doubles, read before the call returns
        check(self.lib.effq_prep_quantiles(_ptr(x), Cc, x.numel() // Cc, mode, (C.c_double * len(q))(*q), len(q),
                                           _ptr(count), _ptr(stats), _ptr(ws), ws.numel(), self.stream),
              "effq_prep_quantiles")
        return count, stats

    def prep_window_mask(self, x: torch.Tensor, lo: float, hi: float, mask: str = "nonzero") -> torch.Tensor:
        """Clip the voxels of the float32 tensor `x` (one modality's plane) that lie inside the mask to [lo, hi] in place
        and leave the others alone (effq_prep_mask_window: a NaN stays; with 'all' it is prep_window)."""
        mode = _flat_f32(self, "prep_window_mask", x, lo, hi, mask)      # the mask is refused before the bounds
        check(self.lib.effq_prep_mask_window(_ptr(x), x.numel(), float(lo), float(hi), mode, self.stream),
              "effq_prep_mask_window")
        return x

    def prep_resample(self, x: torch.Tensor, factors, out_shape, nearest: bool = False) -> torch.Tensor:
        """N x D x H x W volumes on a grid of another spacing (effq_prep_resample): `factors` = target spacing / source
        spacing per axis, `out_shape` the output extents (prep.resample_extent).  float32 volumes are interpolated
        trilinearly; with `nearest` the volumes are uint8 labels and keep their values."""
        x, N, D, H, W = self._prep_volumes("prep_resample", x, torch.uint8 if nearest else torch.float32, limit_c=False)
        f, o = _resample_geometry("prep_resample", factors, out_shape, N)
        y = torch.empty((N,) + o, dtype=x.dtype, device=self.device)
        check(self.lib.effq_prep_resample(_ptr(x), N, D, H, W, f[0], f[1], f[2],
                                          _lib.PREP_NEAREST if nearest else _lib.PREP_LINEAR, _ptr(y), o[0], o[1], o[2],
                                          self.stream), "effq_prep_resample")
        return y

    def prep_resample_cubic(self, x: torch.Tensor, factors, out_shape, keep_zero: bool = False) -> torch.Tensor:
        """N x D x H x W float32 volumes on a grid of another spacing by cubic B-spline interpolation
        (effq_prep_resample_cubic; the rule of prep.py's --prep_interp cubic): `factors` and `out_shape` as in
        prep_resample.  `keep_zero`: an output voxel whose trilinear footprint in `x` is all exactly 0 is +0.0.  The
        fp64 coefficients live in a workspace of 8 B per voxel of `x`; `x` is not modified.  A new tensor."""
        x, N, D, H, W = self._prep_volumes("prep_resample_cubic", x, limit_c=False)
        f, o = _resample_geometry("prep_resample_cubic", factors, out_shape, N)
        y = torch.empty((N,) + o, dtype=torch.float32, device=self.device)
        need = C.c_size_t()
        check(self.lib.effq_prep_cubic_ws_bytes(N, D, H, W, C.byref(need)), "effq_prep_cubic_ws_bytes")
        ws = self._workspace("prep_cubic", need.value)
        check(self.lib.effq_prep_resample_cubic(_ptr(x), N, D, H, W, f[0], f[1], f[2], int(bool(keep_zero)), _ptr(y),
                                                o[0], o[1], o[2], _ptr(ws), ws.numel(), self.stream),
              "effq_prep_resample_cubic")
        return y

    def prep_cubic_plan(self, shape, out_shape) -> dict:
        """How prep_resample_cubic walks N x D x H x W volumes resampled to `out_shape` (effq_prep_cubic_plan; launches
        nothing): chunk and tile_rows of the W prefilter pass, and per launch ('d', 'h', 'w', 'eval') its work items and
        how many of them one trip of its grid covers."""
        n, d, h, w = (int(v) for v in shape)
        o = tuple(int(v) for v in out_shape)
        chunk, rows = C.c_int(), C.c_int()
        items, trip = (C.c_longlong * 4)(), (C.c_longlong * 4)()
        check(self.lib.effq_prep_cubic_plan(n, d, h, w, o[0], o[1], o[2], C.addressof(chunk), C.addressof(rows),
                                            C.addressof(items), C.addressof(trip)),
              "effq_prep_cubic_plan")
        names = ("d", "h", "w", "eval")
        return dict(chunk=chunk.value, tile_rows=rows.value, items=dict(zip(names, (int(v) for v in items))),
                    trip=dict(zip(names, (int(v) for v in trip))))

    def prep_spline_prefilter(self, x: torch.Tensor, passes: str = "dhw", out: Optional[torch.Tensor] = None):
        """The B-spline coefficients of N x D x H x W float32 volumes as a float64 tensor (effq_prep_spline_prefilter), or
        some of the passes alone: 'd' reads `x` and writes `out` (a new tensor unless given), 'h' and 'w' filter `out` in
        place, so without 'd' the caller passes the `out` of an earlier call (`x` gives the shape only)."""
        x, N, D, H, W = self._prep_volumes("prep_spline_prefilter", x, limit_c=False)
        mask = sum(_lib.PREP_SPLINE_PASSES.get(c, 8) for c in set(passes))
        if not 0 < mask <= 7:
            raise _lib.EffqError(f"prep_spline_prefilter: passes {passes!r}: letters of d, h, w")
        if out is None:
            if not mask & 1:
                raise _lib.EffqError("prep_spline_prefilter: the passes h and w work in place: they need `out`")
            out = torch.empty(x.shape, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or \
                self._elsewhere(out):
            raise _lib.EffqError(f"prep_spline_prefilter: `out` must be a contiguous float64 tensor of {tuple(x.shape)}")
        check(self.lib.effq_prep_spline_prefilter(_ptr(x), N, D, H, W, mask, _ptr(out), out.numel() * 8, self.stream),
              "effq_prep_spline_prefilter")
        return out

    def prep_smooth(self, x: torch.Tensor, sigmas, keep_zero: bool = False) -> torch.Tensor:
        """The anti-alias filter of --prep_antialias (effq_prep_smooth): N x D x H x W float32 volumes filtered along
        D, H, W with Gaussians of `sigmas` (voxels; prep.antialias_sigma of the resampling factors), the taps and radii
        from prep.antialias_taps, edges replicated.  `keep_zero`: a voxel that is exactly 0 in `x` is +0.0 in the result.
        A new tensor; `x` itself when every radius is 0.  A NaN or an Inf spreads over its stencil."""
        from . import prep
        x, N, D, H, W = self._prep_volumes("prep_smooth", x, limit_c=False)
        s = tuple(float(v) for v in sigmas)
        if len(s) != 3 or not all(0.0 <= v < float("inf") for v in s):
            raise _lib.EffqError(f"prep_smooth: sigmas {s}: needs three finite values >= 0 (d, h, w)")
        taps = [prep.antialias_taps(v) for v in s]
        radii = [len(t) - 1 for t in taps]
        if max(radii) > _lib.PREP_SMOOTH_MAX_RADIUS:
            raise _lib.EffqError(f"prep_smooth: sigmas {s} give the radii {radii}, at most {_lib.PREP_SMOOTH_MAX_RADIUS}")
        if max(radii) == 0:
            return x
        y = torch.empty_like(x)
        tmp = torch.empty_like(x) if sum(r > 0 for r in radii) > 1 else None
        # the taps are contiguous float32 host arrays, r + 1 each, read before the call returns
        check(self.lib.effq_prep_smooth(_ptr(x), N, D, H, W, taps[0].ctypes.data, radii[0], taps[1].ctypes.data, radii[1],
                                        taps[2].ctypes.data, radii[2], int(bool(keep_zero)), _ptr(y), _ptr(tmp),
                                        self.stream), "effq_prep_smooth")
        return y

    def prep_bbox_moments(self, x: torch.Tensor, mask: str = "nonzero"):
        """Pass 1 over one subject (effq_prep_bbox_moments), x = C x D x H x W float32.  Returns (bbox, count, sum):
        bbox int32[6] = the least d, h, w and the greatest d, h, w of the union of the modalities' masks (least > greatest
        when it is empty), count int64[C] and sum float64[C] over each modality's own mask.  mask 'nonzero': x_c != 0;
        'all': every voxel, the box is the grid."""
        x, Cc, D, H, W = self._prep_volumes("prep_bbox_moments", x)
        mode = self._prep_mask("prep_bbox_moments", mask)
        bbox = torch.empty(6, dtype=torch.int32, device=self.device)
        count = torch.empty(Cc, dtype=torch.int64, device=self.device)
        total = torch.empty(Cc, dtype=torch.float64, device=self.device)
        ws = self._workspace("prep", _lib.PREP_WS_BYTES)
        check(self.lib.effq_prep_bbox_moments(_ptr(x), Cc, D, H, W, mode, _ptr(bbox), _ptr(count), _ptr(total), _ptr(ws),
                                              ws.numel(), self.stream), "effq_prep_bbox_moments")
        return bbox, count, total

    def prep_sqdev(self, x: torch.Tensor, mean, mask: str = "nonzero") -> torch.Tensor:
        """Pass 2 (effq_prep_sqdev): float64[C] = the sum over each modality's mask of (double(x) - mean[c])^2."""
        x, Cc, D, H, W = self._prep_volumes("prep_sqdev", x)
        mode = self._prep_mask("prep_sqdev", mask)
        mu = self._prep_stats("prep_sqdev", mean, Cc)
        out = torch.empty(Cc, dtype=torch.float64, device=self.device)
        ws = self._workspace("prep", _lib.PREP_WS_BYTES)
        check(self.lib.effq_prep_sqdev(_ptr(x), Cc, D * H * W, mode, _ptr(mu), _ptr(out), _ptr(ws), ws.numel(),
                                       self.stream), "effq_prep_sqdev")
        return out

    def prep_standardise_crop(self, x: torch.Tensor, pmin, pmax, mean, std, mask: str = "nonzero") -> torch.Tensor:
        """Pass 3 (effq_prep_standardise_crop): the box pmin <= (d, h, w) < pmax of every modality as
        float((double(x) - mean[c]) / std[c]) inside the modality's mask and +0.0 outside it."""
        x, Cc, D, H, W = self._prep_volumes("prep_standardise_crop", x)
        mode = self._prep_mask("prep_standardise_crop", mask)
        lo, hi, clo, chi = self._prep_box("prep_standardise_crop", (D, H, W), pmin, pmax)
        mu, sd = self._prep_stats("prep_standardise_crop", mean, Cc), self._prep_stats("prep_standardise_crop", std, Cc)
        y = torch.empty((Cc,) + tuple(b - a for a, b in zip(lo, hi)), dtype=torch.float32, device=self.device)
        check(self.lib.effq_prep_standardise_crop(_ptr(x), Cc, D, H, W, mode, clo, chi, _ptr(mu), _ptr(sd), _ptr(y),
                                                  self.stream), "effq_prep_standardise_crop")
        return y

    def prep_crop_u8(self, x: torch.Tensor, pmin, pmax) -> torch.Tensor:
        """The box pmin <= (d, h, w) < pmax of C x D x H x W uint8 volumes (effq_prep_crop_u8: the label)."""
        x, Cc, D, H, W = self._prep_volumes("prep_crop_u8", x, torch.uint8, limit_c=False)
        lo, hi, clo, chi = self._prep_box("prep_crop_u8", (D, H, W), pmin, pmax)
        y = torch.empty((Cc,) + tuple(b - a for a, b in zip(lo, hi)), dtype=torch.uint8, device=self.device)
        check(self.lib.effq_prep_crop_u8(_ptr(x), Cc, D, H, W, clo, chi, _ptr(y), self.stream), "effq_prep_crop_u8")
        return y

    def prep_union_mask(self, x: torch.Tensor, mask: str = "nonzero") -> torch.Tensor:
        """D x H x W uint8, 1 where the mask of any modality of x (C x D x H x W) holds (effq_prep_union_mask)."""
        x, Cc, D, H, W = self._prep_volumes("prep_union_mask", x)
        mode = self._prep_mask("prep_union_mask", mask)
        m = torch.empty((D, H, W), dtype=torch.uint8, device=self.device)
        check(self.lib.effq_prep_union_mask(_ptr(x), Cc, D * H * W, mode, _ptr(m), self.stream), "effq_prep_union_mask")
        return m

    @staticmethod
    def _orient_plan(what: str, src_axis, flip):
        """(ctypes int[3], flip mask) of a plan: `flip` is three truth values, one per output axis."""
        try:
            axes, fl = tuple(int(a) for a in src_axis), tuple(bool(f) for f in flip)
        except (TypeError, ValueError):
            axes, fl = (), ()
        if sorted(axes) != [0, 1, 2] or len(fl) != 3:
            raise _lib.EffqError(f"{what}: src_axis {src_axis!r} must be a permutation of 0, 1, 2 and flip {flip!r} three "
                                 f"truth values")
        return axes, (C.c_int * 3)(*axes), sum(1 << p for p in range(3) if fl[p])

    def prep_reorient_variant(self, src_axis, flip, elem_bytes: int) -> int:
        """The kernel effq_prep_reorient would launch for this plan (effq_prep_reorient_plan): 0 rows, 1 tiled transpose."""
        _, cax, mask = self._orient_plan("prep_reorient_variant", src_axis, flip)
        v = C.c_int(-1)
        check(self.lib.effq_prep_reorient_plan(cax, mask, int(elem_bytes), C.byref(v)), "effq_prep_reorient_plan")
        return int(v.value)

    def prep_reorient(self, x: torch.Tensor, src_axis, flip) -> torch.Tensor:
        """N x D x H x W (or D x H x W) float32 or uint8 volumes with their axes permuted and reversed
        (effq_prep_reorient): output axis p is source axis src_axis[p], reversed iff flip[p]; a new tensor, bit for bit
        numpy.flip(numpy.transpose(x)).  The tensor must be contiguous in its own storage; a uint8 one may start at any
        byte of a larger buffer."""
        if x.dim() not in (3, 4) or x.dtype not in (torch.float32, torch.uint8) or x.numel() == 0 or \
                not x.is_contiguous() or self._elsewhere(x):
            raise _lib.EffqError(f"prep_reorient: needs a contiguous [N x] D x H x W float32 or uint8 tensor on "
                                 f"{self.device}, got {tuple(x.shape)} {x.dtype} on {x.device}")
        axes, cax, mask = self._orient_plan("prep_reorient", src_axis, flip)
        dims = tuple(int(n) for n in x.shape[-3:])
        N = int(x.shape[0]) if x.dim() == 4 else 1
        if x.numel() >= 2 ** 31 or max(dims) > 32767:
            raise _lib.EffqError(f"prep_reorient: shape {tuple(x.shape)}: 2^31 - 1 voxels in all and 32767 along an axis "
                                 f"at most")
        out = tuple(dims[a] for a in axes)
        y = torch.empty(((N,) if x.dim() == 4 else ()) + out, dtype=x.dtype, device=x.device)
        check(self.lib.effq_prep_reorient(_ptr(x), N, dims[0], dims[1], dims[2], cax, mask, x.element_size(), _ptr(y),
                                          self.stream), "effq_prep_reorient")
        return y
