"""The device steps of the one-pass calibrator (effq_gptq_chol, effq_gptq_sweep; the rule of gptq.py and of --qconv gptq):
free functions over a HipOps, as those of ops_crf are."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr

BLOCK = 64        # gptq.hip: columns per block of the factor and of the sweep
LEVELS_MAX = 256  # csrc/fp_level.h (FP_LEVELS_MAX)


def _npad(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK * BLOCK


def gptq_plan(ops, c2: int, n: int) -> dict:
    """The launches gptq_chol and gptq_sweep make for c2 rows of n unknowns (effq_gptq_plan_query; launches nothing)."""
    out = [C.c_int() for _ in range(6)]
    check(ops.lib.effq_gptq_plan_query(int(c2), int(n), *[C.byref(o) for o in out]), "effq_gptq_plan_query")
    return dict(zip(("nblk", "chol_launches", "chol_tiles", "sweep_launches", "block_grid", "trail_gy"),
                    (o.value for o in out)))


def gptq_chol(ops, A0: torch.Tensor, eta: float, read_flag: bool = False) -> torch.Tensor:
    """The fp64 factor of H = A0 + eta I = P P^T, P upper triangular, in the sweep's layout (include/effq_hip.h): a flat
    fp64 tensor, gptq_factor() gives the dense P and gptq_flag() the "not positive definite" word.  read_flag: read that
    word now (one host synchronisation) and raise EffqError when it is set; otherwise nothing is read."""
    if not isinstance(A0, torch.Tensor) or A0.dim() != 2 or A0.shape[0] != A0.shape[1] or A0.numel() == 0:
        raise _lib.EffqError(f"gptq_chol: A0 needs a square matrix, got {tuple(getattr(A0, 'shape', ()))}")
    A0 = ops._f32(A0)
    n = int(A0.shape[0])
    nbytes = ops.lib.effq_gptq_factor_bytes(n)
    if nbytes == 0:
        raise _lib.EffqError(f"gptq_chol: n = {n} is outside what the factorisation takes")
    P = torch.empty(nbytes // 8, dtype=torch.float64, device=ops.device)
    ws = ops._workspace("gptq_chol", ops.lib.effq_gptq_chol_ws_bytes(n))
    check(ops.lib.effq_gptq_chol(_ptr(A0), float(eta), n, _ptr(P), nbytes, _ptr(ws), ws.numel(), int(bool(read_flag)),
                                 ops.stream), "effq_gptq_chol")
    return P


def gptq_flag(P: torch.Tensor, n: int) -> torch.Tensor:
    """The flag word of a factor as a 1-element int32 device tensor (0: factored; 1: not positive definite)."""
    m = _npad(n) ** 2
    return P[m:m + 1].view(torch.int32)[:1]


def gptq_factor(P: torch.Tensor, n: int) -> torch.Tensor:
    """The dense n x n upper-triangular P of a factor (tests, diagnostics): P[i][j] = L[n-1-i][n-1-j]."""
    npad = _npad(n)
    return P[:npad * npad].view(npad, npad)[:n, :n].flip(0, 1)


def gptq_sweep(ops, P: torch.Tensor, n: int, u_w: torch.Tensor, u_b: Optional[torch.Tensor], alpha: torch.Tensor,
               levels: int, want_ids: bool = False, out=None, per_row: Optional[bool] = None):
    """(G, b, ids, err, row_flag): the sweep of gptq.py over the factor `P` of gptq_chol for the continuous optimum
    u_w (c2, n - has_bias), u_b (c2) or None, fp32; alpha: 1 or c2 device doubles (per_row says which where c2 = 1).  G (c2, nw) and b (c2) fp32, ids uint8
    like G (want_ids), err (c2) doubles, row_flag (c2) int32.  out: (G, b, ids, err, row_flag) to write into instead of
    new tensors.  Nothing is read back; a factor whose flag is set leaves every output as it is."""
    what = "gptq_sweep"
    has_b = u_b is not None
    nw = int(n) - int(has_b)
    if not isinstance(u_w, torch.Tensor) or u_w.dim() != 2 or u_w.shape[1] != nw or u_w.shape[0] < 1:
        raise _lib.EffqError(f"{what}: u_w needs (c2, {nw}), got {tuple(getattr(u_w, 'shape', ()))}")
    c2 = int(u_w.shape[0])
    u_w = ops._f32(u_w)
    if has_b:
        u_b = ops._f32(u_b)
        if u_b.numel() != c2:
            raise _lib.EffqError(f"{what}: u_b has {u_b.numel()} elements for {c2} rows")
    if P.dtype != torch.float64 or ops._elsewhere(P) or P.numel() * 8 != ops.lib.effq_gptq_factor_bytes(int(n)) or \
            P.numel() == 0 or not P.is_contiguous():
        raise _lib.EffqError(f"{what}: P is not the factor gptq_chol returns for n = {n}")
    if per_row is None:
        per_row = alpha.numel() == c2 and c2 > 1
    if alpha.dtype != torch.float64 or ops._elsewhere(alpha) or alpha.numel() != (c2 if per_row else 1) or not alpha.is_contiguous():
        raise _lib.EffqError(f"{what}: alpha needs {c2 if per_row else 1} device double(s)")
    if not 2 <= int(levels) <= LEVELS_MAX:
        raise _lib.EffqError(f"{what}: {levels} levels, takes 2 .. {LEVELS_MAX}")
    dev = ops.device
    if out is None:
        out = (torch.empty(c2, nw, dtype=torch.float32, device=dev),
               torch.empty(c2, dtype=torch.float32, device=dev) if has_b else None,
               torch.empty(c2, nw, dtype=torch.uint8, device=dev) if want_ids else None,
               torch.empty(c2, dtype=torch.float64, device=dev), torch.empty(c2, dtype=torch.int32, device=dev))
    G, b, ids, err, row_flag = out
    for name, t, dt, m in (("G", G, torch.float32, c2 * nw), ("b", b, torch.float32, c2), ("ids", ids, torch.uint8, c2 * nw),
                           ("err", err, torch.float64, c2), ("row_flag", row_flag, torch.int32, c2)):
        if t is None and (name == "ids" or (name == "b" and not has_b)):
            continue
        if t is None or t.dtype != dt or t.numel() != m or not t.is_contiguous() or ops._elsewhere(t):
            raise _lib.EffqError(f"{what}: {name} needs {m} contiguous {dt} values on {ops.device}")
    ws = ops._workspace("gptq", ops.lib.effq_gptq_ws_bytes(c2, int(n)))
    check(ops.lib.effq_gptq_sweep(_ptr(P), int(n), _ptr(u_w), _ptr(u_b), c2, int(has_b), _ptr(alpha),
                                  int(bool(per_row)), int(levels), _ptr(G), _ptr(b), _ptr(ids), _ptr(err),
                                  _ptr(row_flag), _ptr(ws), ws.numel(), ops.stream), "effq_gptq_sweep")
    return G, b, ids, err, row_flag
