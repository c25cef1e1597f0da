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


REFINE_MAX_PASSES = 16  # gptq_refine.hip (GR_MAX_PASSES)


def gptq_refine_plan(ops, c2: int, n: int, passes: int) -> dict:
    """The launches gptq_refine makes for c2 rows of n unknowns (effq_gptq_refine_plan_query; launches nothing)."""
    out = [C.c_int() for _ in range(5)]
    check(ops.lib.effq_gptq_refine_plan_query(int(c2), int(n), int(passes), *[C.byref(o) for o in out]),
          "effq_gptq_refine_plan_query")
    return dict(zip(("nblk", "launches", "block_grid", "update_gx", "update_gy"), (o.value for o in out)))


def gptq_refine(ops, A0: torch.Tensor, eta: float, u_w: torch.Tensor, u_b: Optional[torch.Tensor], alpha: torch.Tensor,
                levels: int, passes: int, G: torch.Tensor, b: Optional[torch.Tensor], ids: torch.Tensor,
                row_flag: torch.Tensor, pd_flag: torch.Tensor, per_row: Optional[bool] = None, out=None):
    """(err, moves): `passes` coordinate-descent passes of gptq.refine_host over what gptq_sweep left in G, b and ids
    (want_ids), which are updated in place; A0 and eta are those of the factor the sweep ran on, pd_flag its gptq_flag,
    row_flag the sweep's.  err (c2) doubles: the final (q - u*) H (q - u*)^T; moves (c2) int32: accepted weight moves.
    out: (err, moves) to write into.  Nothing is read back; a set flag leaves every output as it is."""
    what = "gptq_refine"
    has_b = u_b is not None
    if not isinstance(A0, torch.Tensor) or A0.dim() != 2 or A0.shape[0] != A0.shape[1] or A0.numel() == 0:
        raise _lib.EffqError(f"{what}: A0 needs a square matrix, got {tuple(getattr(A0, 'shape', ()))}")
    A0 = ops._f32(A0)
    n = int(A0.shape[0])
    nw = n - int(has_b)
    if not isinstance(u_w, torch.Tensor) or u_w.dim() != 2 or u_w.shape[1] != nw or u_w.shape[0] < 1:
        raise _lib.EffqError(f"{what}: u_w needs (c2, {nw}), got {tuple(getattr(u_w, 'shape', ()))}")
    c2 = int(u_w.shape[0])
    u_w = ops._f32(u_w)
    if has_b:
        u_b = ops._f32(u_b)
        if u_b.numel() != c2:
            raise _lib.EffqError(f"{what}: u_b has {u_b.numel()} elements for {c2} rows")
    if per_row is None:
        per_row = alpha.numel() == c2 and c2 > 1
    if alpha.dtype != torch.float64 or ops._elsewhere(alpha) or alpha.numel() != (c2 if per_row else 1) or not alpha.is_contiguous():
        raise _lib.EffqError(f"{what}: alpha needs {c2 if per_row else 1} device double(s)")
    if not 2 <= int(levels) <= LEVELS_MAX:
        raise _lib.EffqError(f"{what}: {levels} levels, takes 2 .. {LEVELS_MAX}")
    if not 1 <= int(passes) <= REFINE_MAX_PASSES:
        raise _lib.EffqError(f"{what}: {passes} passes, takes 1 .. {REFINE_MAX_PASSES}")
    dev = ops.device
    if out is None:
        out = (torch.empty(c2, dtype=torch.float64, device=dev), torch.empty(c2, dtype=torch.int32, device=dev))
    err, moves = out
    for name, t, dt, m in (("G", G, torch.float32, c2 * nw), ("b", b, torch.float32, c2), ("ids", ids, torch.uint8, c2 * nw),
                           ("err", err, torch.float64, c2), ("moves", moves, torch.int32, c2),
                           ("row_flag", row_flag, torch.int32, c2), ("pd_flag", pd_flag, torch.int32, 1)):
        if t is None and name == "b" and not has_b:
            continue
        if t is None or t.dtype != dt or t.numel() != m or not t.is_contiguous() or ops._elsewhere(t):
            raise _lib.EffqError(f"{what}: {name} needs {m} contiguous {dt} values on {ops.device}")
    ws = ops._workspace("gptq_refine", ops.lib.effq_gptq_refine_ws_bytes(c2, n))
    check(ops.lib.effq_gptq_refine(_ptr(A0), float(eta), n, _ptr(u_w), _ptr(u_b), c2, int(has_b), _ptr(alpha),
                                   int(bool(per_row)), int(levels), int(passes), _ptr(G), _ptr(b), _ptr(ids), _ptr(err),
                                   _ptr(moves), _ptr(row_flag), _ptr(pd_flag), _ptr(ws), ws.numel(), ops.stream),
          "effq_gptq_refine")
    return err, moves


RESCALE_MAX_ROUNDS = 8  # gptq.py: rounds of [refit, passes]


def gptq_rescale_plan(ops, c2: int, n: int) -> dict:
    """The launches gptq_rescale makes for c2 rows of n unknowns (effq_gptq_rescale_plan_query; launches nothing)."""
    out = [C.c_int() for _ in range(6)]
    check(ops.lib.effq_gptq_rescale_plan_query(int(c2), int(n), *[C.byref(o) for o in out]), "effq_gptq_rescale_plan_query")
    return dict(zip(("nblk", "tiles", "tiles_per_run", "runs", "forms_grid", "launches"), (o.value for o in out)))


def gptq_rescale(ops, A0: torch.Tensor, eta: float, u_w: torch.Tensor, u_b: Optional[torch.Tensor], alpha: torch.Tensor,
                 levels: int, G: torch.Tensor, b: Optional[torch.Tensor], ids: torch.Tensor, row_flag: torch.Tensor,
                 pd_flag: torch.Tensor, per_row: Optional[bool] = None, out=None):
    """(err, kept): the scale (and the bias) refitted on H = A0 + eta I with the ids fixed, the rule of gptq.rescale_host,
    over what gptq_sweep or gptq_refine left: alpha (1 or c2 device doubles), G and b are updated in place, ids only read.
    err (c2) doubles: f at the point every row now stands on; kept (1) int32: incremented for every refit not taken.
    out: (err, kept) to write into (kept is not cleared).  Nothing is read back; a set flag leaves every output as it is."""
    what = "gptq_rescale"
    has_b = u_b is not None
    if not isinstance(A0, torch.Tensor) or A0.dim() != 2 or A0.shape[0] != A0.shape[1] or A0.numel() == 0:
        raise _lib.EffqError(f"{what}: A0 needs a square matrix, got {tuple(getattr(A0, 'shape', ()))}")
    A0 = ops._f32(A0)
    n = int(A0.shape[0])
    nw = n - int(has_b)
    if not isinstance(u_w, torch.Tensor) or u_w.dim() != 2 or u_w.shape[1] != nw or u_w.shape[0] < 1:
        raise _lib.EffqError(f"{what}: u_w needs (c2, {nw}), got {tuple(getattr(u_w, 'shape', ()))}")
    c2 = int(u_w.shape[0])
    u_w = ops._f32(u_w)
    if has_b:
        u_b = ops._f32(u_b)
        if u_b.numel() != c2:
            raise _lib.EffqError(f"{what}: u_b has {u_b.numel()} elements for {c2} rows")
    if per_row is None:
        per_row = alpha.numel() == c2 and c2 > 1
    if alpha.dtype != torch.float64 or ops._elsewhere(alpha) or alpha.numel() != (c2 if per_row else 1) or not alpha.is_contiguous():
        raise _lib.EffqError(f"{what}: alpha needs {c2 if per_row else 1} device double(s)")
    if not 2 <= int(levels) <= LEVELS_MAX:
        raise _lib.EffqError(f"{what}: {levels} levels, takes 2 .. {LEVELS_MAX}")
    dev = ops.device
    if out is None:
        out = (torch.empty(c2, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
    err, kept = out
    for name, t, dt, m in (("G", G, torch.float32, c2 * nw), ("b", b, torch.float32, c2), ("ids", ids, torch.uint8, c2 * nw),
                           ("err", err, torch.float64, c2), ("kept", kept, torch.int32, 1),
                           ("row_flag", row_flag, torch.int32, c2), ("pd_flag", pd_flag, torch.int32, 1)):
        if t is None and name == "b" and not has_b:
            continue
        if t is None or t.dtype != dt or t.numel() != m or not t.is_contiguous() or ops._elsewhere(t):
            raise _lib.EffqError(f"{what}: {name} needs {m} contiguous {dt} values on {ops.device}")
    ws = ops._workspace("gptq_rescale", ops.lib.effq_gptq_rescale_ws_bytes(c2, n))
    check(ops.lib.effq_gptq_rescale(_ptr(A0), float(eta), n, _ptr(u_w), _ptr(u_b), c2, int(has_b), _ptr(ids), int(levels),
                                    int(bool(per_row)), _ptr(row_flag), _ptr(pd_flag), _ptr(alpha), _ptr(G), _ptr(b),
                                    _ptr(err), _ptr(kept), _ptr(ws), ws.numel(), ops.stream), "effq_gptq_rescale")
    return err, kept


def gptq_order(A0: torch.Tensor, has_bias: bool) -> torch.Tensor:
    """The permutation of gptq.order_host on the device, nothing read back: the weight columns by descending diag(A0),
    ties in their own order, the bias last."""
    n = int(A0.shape[0])
    nw = n - int(bool(has_bias))
    perm = torch.argsort(A0.diagonal()[:nw], descending=True, stable=True)
    return torch.cat([perm, torch.arange(nw, n, device=A0.device)]) if has_bias else perm
