"""The device steps of the bias field correction (effq_prep_bias_log, _hist, _fit, _apply; the rule of bias.py and of
prep.py's --prep_bias): free functions over a HipOps, as those of ops_register are."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr
from .ops_register import _volume

BINS, LEVELS, LATTICE = _lib.PREP_BIAS_BINS, _lib.PREP_BIAS_LEVELS, _lib.PREP_BIAS_LATTICE
LATTICE_OFFSETS = tuple(int(sum((2 ** k + 3) ** 3 for k in range(l))) for l in range(LEVELS + 1))   # 0, 64, 189, 532, 1863


def sample_shape(dims, stride, offset) -> tuple:
    """The samples per axis: the indices s q + o below the extent."""
    return tuple((n - o + s - 1) // s for n, s, o in zip(dims, stride, offset))


def _samples(what: str, dims, stride, offset):
    try:
        s, o = tuple(int(v) for v in stride), tuple(int(v) for v in offset)
    except (TypeError, ValueError) as e:
        raise _lib.EffqError(f"{what}: stride or offset: {e}") from e
    if len(s) != 3 or len(o) != 3 or min(s) < 1 or any(not 0 <= b < n for b, n in zip(o, dims)):
        raise _lib.EffqError(f"{what}: stride {s}, offset {o}: three strides >= 1 and three offsets inside {dims}")
    return (C.c_int * 3)(*s), (C.c_int * 3)(*o), sample_shape(dims, s, o)


def _tensor(ops, what: str, name: str, t, dtype, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() \
            or ops._elsewhere(t):
        raise _lib.EffqError(f"{what}: {name} needs a contiguous {tuple(shape)} {dtype} tensor on {ops.device}, got "
                             f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
    return t


def _decode(code: int) -> float:
    """The float of the order-preserving uint32 code of effq_hip.h."""
    bits = (code & 0x7FFFFFFF) if code & 0x80000000 else (~code & 0xFFFFFFFF)
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def prep_bias_log(ops, v: torch.Tensor, mask: str = "nonzero"):
    """(u, m) of the D x H x W float32 scan `v`: m (uint8) is 1 where v lies in `mask`, is finite and > 0; u (float32) is
    log(v) there, formed in fp64 and rounded once, and 0 elsewhere."""
    what = "prep_bias_log"
    dims = _volume(ops, what, v, torch.float32)
    if mask not in _lib.PREP_MASKS:
        raise _lib.EffqError(f"{what}: mask {mask!r}, one of {', '.join(_lib.PREP_MASKS)}")
    u, m = torch.empty_like(v), torch.empty(dims, dtype=torch.uint8, device=ops.device)
    check(ops.lib.effq_prep_bias_log(_ptr(v), *dims, _lib.PREP_MASKS[mask], _ptr(u), _ptr(m), ops.stream),
          "effq_prep_bias_log")
    return u, m


def prep_bias_hist(ops, u, m, f, stride, offset):
    """(counters, lo, hi, n) of r = u - f over the samples of `m`: n their number, lo and hi the fp32 min and max of r,
    counters the BINS int64 of the linear split between the bin centres in units of 1 / 65536 (all 0 when hi == lo).
    Host values: the call reads them back."""
    what = "prep_bias_hist"
    dims = _volume(ops, what, u, torch.float32)
    s, o, shape = _samples(what, dims, stride, offset)
    _tensor(ops, what, "m", m, torch.uint8, dims)
    _tensor(ops, what, "f", f, torch.float32, shape)
    hist = torch.empty(BINS + 2, dtype=torch.int64, device=ops.device)
    check(ops.lib.effq_prep_bias_hist(_ptr(u), _ptr(m), _ptr(f), *dims, s, o, _ptr(hist), ops.stream),
          "effq_prep_bias_hist")
    got = hist.cpu().numpy()
    n, packed = int(got[BINS + 1]), int(got[BINS]) & 0xFFFFFFFFFFFFFFFF
    if n == 0:
        return got[:BINS].copy(), 0.0, 0.0, 0
    return got[:BINS].copy(), _decode(packed & 0xFFFFFFFF), _decode(packed >> 32), n


def prep_bias_fit(ops, u, m, f, stride, offset, level: int, lo: float, hi: float, table, phi, lattice):
    """One iteration at `level` with the sharpened `table` (BINS host doubles over [lo, hi]): `phi` (float64, (n + 3)^3)
    receives the lattice of e = r - lerp(table, r), `lattice` gains it, `f` gains its evaluation on the samples.
    Returns the sums of exp(df) and exp(df)^2 over the samples of `m`, host floats."""
    what = "prep_bias_fit"
    dims = _volume(ops, what, u, torch.float32)
    s, o, shape = _samples(what, dims, stride, offset)
    if not 0 <= int(level) < LEVELS:
        raise _lib.EffqError(f"{what}: level {level}, needs 0 ... {LEVELS - 1}")
    cells = (2 ** int(level) + 3) ** 3
    _tensor(ops, what, "m", m, torch.uint8, dims)
    _tensor(ops, what, "f", f, torch.float32, shape)
    _tensor(ops, what, "phi", phi, torch.float64, (cells,))
    _tensor(ops, what, "lattice", lattice, torch.float64, (cells,))
    e = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1))
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if e.shape[0] != BINS or not np.all(np.isfinite(e)) or not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise _lib.EffqError(f"{what}: needs {BINS} finite table entries and finite lo < hi, got {e.shape[0]} entries, "
                             f"lo {lo}, hi {hi}")
    need = int(ops.lib.effq_bias_fit_ws_bytes(*dims, s, o))
    ws = ops._workspace("prep_bias_fit", need)
    sums = torch.empty(2, dtype=torch.float64, device=ops.device)
    # the table is a host array, read before the call returns
    check(ops.lib.effq_prep_bias_fit(_ptr(u), _ptr(m), _ptr(f), *dims, s, o, int(level), lo, hi, e.ctypes.data, _ptr(phi),
                                     _ptr(lattice), _ptr(sums), _ptr(ws), ws.numel(), ops.stream), "effq_prep_bias_fit")
    s1, s2 = sums.cpu().tolist()
    return s1, s2


def prep_bias_apply(ops, v, m, lattices):
    """(y, lo, hi): y = float32(v / exp(f)) on the full grid, f the sum of the four `lattices` (one float64 tensor of
    LATTICE entries, level after level); lo, hi the min and max of float32(exp(f)) over `m` (inf, -inf for an empty m)."""
    what = "prep_bias_apply"
    dims = _volume(ops, what, v, torch.float32)
    _tensor(ops, what, "m", m, torch.uint8, dims)
    _tensor(ops, what, "lattices", lattices, torch.float64, (LATTICE,))
    y = torch.empty_like(v)
    rng = torch.empty(2, dtype=torch.int32, device=ops.device)
    check(ops.lib.effq_prep_bias_apply(_ptr(v), _ptr(m), *dims, _ptr(lattices), _ptr(y), _ptr(rng), ops.stream),
          "effq_prep_bias_apply")
    lo, hi = (int(c) & 0xFFFFFFFF for c in rng.cpu().tolist())
    if lo == 0xFFFFFFFF and hi == 0:
        return y, float("inf"), float("-inf")
    return y, _decode(lo), _decode(hi)
