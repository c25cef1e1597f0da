"""The lesion pairs of one case (effq_seg_lesion_match): a free function over a HipOps, which keeps the surface of HipOps
and of its mixins what it is."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops_base import _ptr


def seg_lesion_match(ops, logits: torch.Tensor, label: torch.Tensor, task: str, fuse: Optional[str] = None,
                     max_rows: Optional[int] = None, max_pairs: Optional[int] = None):
    """The lesions of one case and the overlap of every pair of them (effq_seg_lesion_match), arguments and decisions as
    ops.seg_lesion_table.  Returns (counts, nrows, rows, pairs) on the host: counts, nrows and rows are bit for bit
    seg_lesion_table's; pairs is a list of C int32 tensors n_c x 3 = label row, predicted row (0-based rows of `rows`:
    of plane C + c and of plane c), the voxels both lesions hold - one record per label lesion and predicted lesion of
    class c that share a voxel, ascending in (label row, predicted row).  max_rows as cc_table; max_pairs: the pairs per
    class asked for first (default _lib.LESION_PAIR_ROWS).  A plane with more components than max_rows costs one more
    call with the capacity the row counts give, a class with more pairs than max_pairs one more with twice as many,
    until every class fits: all rows and all pairs are returned."""
    what = "seg_lesion_match"
    x, lab, Cc, (D, H, W), mode, fcode, thresh = ops._seg_case(what, logits, label, task, fuse, True)
    P = 2 * Cc
    if D * H * W == 0 or P * D * H * W >= 2 ** 31:
        raise _lib.EffqError(f"{what}: {P} masks of {D * H * W} voxels (2^31 - 1 voxels in all at most)")
    cap = _lib.LESION_TABLE_ROWS if max_rows is None else int(max_rows)
    capp = _lib.LESION_PAIR_ROWS if max_pairs is None else int(max_pairs)
    if cap <= 0:
        raise _lib.EffqError(f"{what}: max_rows {max_rows}, needs a positive capacity")
    if capp <= 0:
        raise _lib.EffqError(f"{what}: max_pairs {max_pairs}, needs a positive capacity")
    head = 4 * Cc                                  # int64 words: counts, then nrows (P), then npairs (C)
    front = 2 * (head + P + Cc)
    while True:
        if P * cap * 3 >= 2 ** 31 or Cc * capp * 3 >= 2 ** 31:
            raise _lib.EffqError(f"{what}: tables of {P} x {cap} rows and {Cc} x {capp} pairs")
        # one int32 buffer, so that one copy brings all of it to the host
        buf = torch.empty(front + P * cap * 3 + Cc * capp * 3, dtype=torch.int32, device=ops.device)
        base = buf.data_ptr()
        ws = ops._workspace("cc", ops.lib.effq_seg_lesion_match_ws_bytes(Cc, D, H, W, cap, capp))
        check(ops.lib.effq_seg_lesion_match(_ptr(x), _ptr(lab), Cc, D, H, W, mode, fcode, thresh,
                                            _lib.LESION_CONNECTIVITY, cap, capp, C.c_void_p(base),
                                            C.c_void_p(base + 8 * head), C.c_void_p(base + 4 * front),
                                            C.c_void_p(base + 8 * (head + P)),
                                            C.c_void_p(base + 4 * (front + P * cap * 3)), _ptr(ws), ws.numel(),
                                            ops.stream), "effq_seg_lesion_match")
        host = buf.cpu()
        words = host[:front].view(torch.int64)
        nrows, npairs = words[head:head + P], words[head + P:]
        most = int(nrows.max())
        short = bool((npairs < 0).any())
        if most <= cap and not short:
            table = host[front:front + P * cap * 3].view(P, cap, 3)
            ptab = host[front + P * cap * 3:].view(Cc, capp, 3)
            return (words[:head].view(Cc, 4), nrows, [table[q, :int(nrows[q])] for q in range(P)],
                    [ptab[c, :int(npairs[c])] for c in range(Cc)])
        cap = max(cap, most)
        if short:
            capp *= 2
