"""Validation of stitched logits and label maps (evaluate.validate_seg, predict): decisions and their threshold,
tallies, threshold sweep, label maps, agreement with the FP network, connected components and their tables, label
cleaning and both distance transforms (effq_seg_*, effq_cc_*, effq_label_*, effq_edt_*)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops_base import OpsBase, _ptr

_DECISION_MODES = {"lits": _lib.SEG_ARGMAX, "argmax": _lib.SEG_ARGMAX, "brats": _lib.SEG_SIGMOID,
                   "sigmoid": _lib.SEG_SIGMOID}


def _decision_mode(name, accepted, refusal: str) -> int:
    """_lib.SEG_ARGMAX / _lib.SEG_SIGMOID of the task or mode `name`; a caller takes only the spellings in `accepted`
    (a tuple of keys of _DECISION_MODES) and refuses every other with its own `refusal`."""
    if name not in accepted:
        raise _lib.EffqError(refusal)
    return _DECISION_MODES[name]


def _label_rule(what: str, rule: str, fuse, Cc: int) -> int:
    """The merge code of seg_labels and seg_labels_source: a known label rule, and `fuse` checked for it (_fuse_code)."""
    if rule not in _lib.SEG_LABEL_RULES:
        raise _lib.EffqError(f"{what}: unknown rule {rule!r} (one of {', '.join(_lib.SEG_LABEL_RULES)})")
    return SegOps._fuse_code(what, fuse, rule == "argmax", f"rule {rule}", Cc, rule)


def _source_grid(what: str, x: torch.Tensor, pmin, grid, factors, source_shape, planes: int, size_refusal: str):
    """The geometry seg_labels_source and seg_probs_source share, parsed and bounded: the ctypes arrays (pmin int[3],
    grid int[3], factors double[3], source_shape int[3]) their C calls take.  `planes` source grids are allocated by
    the caller, who words the refusal of a size beyond them (`size_refusal`, formatted with src and planes)."""
    try:
        lo, G, src = (tuple(int(v) for v in t) for t in (pmin, grid, source_shape))
        f = (1.0, 1.0, 1.0) if factors is None else tuple(float(v) for v in factors)
    except (TypeError, ValueError) as e:
        raise _lib.EffqError(f"{what}: {e}") from e
    if len(lo) != 3 or len(G) != 3 or len(src) != 3 or len(f) != 3 or x.numel() == 0:
        raise _lib.EffqError(f"{what}: box at {lo} of {tuple(x.shape[1:])}, grid {G}, factors {f}, source "
                             f"{src}: three values each")
    if min(src) < 1 or max(src) > 32767 or planes * math.prod(src) >= 2 ** 31:    # the outputs are not allocated for these
        raise _lib.EffqError(size_refusal.format(src=src, planes=planes))
    i3 = C.c_int * 3
    return i3(*lo), i3(*G), (C.c_double * 3)(*f), i3(*src)


def _connectivity(what: str, connectivity) -> None:
    if connectivity not in (6, 26):
        raise _lib.EffqError(f"{what}: connectivity {connectivity}, 6 or 26")


def _plane_limits(what: str, m: torch.Tensor, P: int, D: int, H: int, W: int) -> None:
    if P > 65535 or m.numel() >= 2 ** 31:
        raise _lib.EffqError(f"{what}: {P} masks of {D * H * W} voxels (at most 65535 masks, 2^31 - 1 voxels in all)")


class SegOps(OpsBase):
    """The validation wrappers of HipOps."""

    def set_decision_threshold(self, logit: Optional[float]) -> None:
        """The logit every sigmoid decision of these ops is taken at from now on (--thresh): sigmoid_threshold() returns
        the fp32 nearest `logit`, so the tallies, the label maps, the lesions, the surfaces and the agreement follow it.
        None: the default again.  seg_sweep and sweep_edges keep the default: the sweep does not depend on it."""
        if logit is None:
            self._decision_thresh = None
            return
        v = float(torch.tensor(float(logit), dtype=torch.float32).item())
        if not math.isfinite(v):
            raise _lib.EffqError(f"set_decision_threshold: {logit!r} is no finite fp32 logit")
        self._decision_thresh = v

    def sigmoid_threshold(self) -> float:
        """The logit a sigmoid decision is taken at: the one set_decision_threshold set, or default_sigmoid_threshold()."""
        if getattr(self, "_decision_thresh", None) is not None:
            return self._decision_thresh
        return self.default_sigmoid_threshold()

    def default_sigmoid_threshold(self) -> float:
        """The least fp32 x at which the framework's fp32 `torch.sigmoid(x) >= 0.5` holds on this device.  Near 0 it is
        not 0: a small negative logit rounds to exactly 0.5.  Found by bisection over the bit patterns of -x, then
        checked on the 2^17 floats around it; cached."""
        if getattr(self, "_sig_thresh", None) is not None:
            return self._sig_thresh

        def decide(mags):       # magnitudes as int32 bit patterns -> decision of sigmoid(-mag) >= 0.5
            x = -torch.tensor(mags, dtype=torch.int32).view(torch.float32).to(self.device)
            return (torch.sigmoid(x) >= 0.5).cpu()

        lo, hi = 0, 0x3F800000            # sigmoid(-0) = 0.5 holds, sigmoid(-1) < 0.5
        while hi - lo > 1:
            cand = sorted({lo + (hi - lo) * k // 4097 for k in range(1, 4097)} - {lo, hi})
            ok = decide(cand)
            bad = (~ok).nonzero()
            first_bad = int(bad[0]) if len(bad) else len(cand)
            lo = cand[first_bad - 1] if first_bad > 0 else lo
            hi = cand[first_bad] if first_bad < len(cand) else hi
        dense = list(range(max(0, lo - (1 << 16)), lo + (1 << 16)))
        if not torch.equal(decide(dense), torch.tensor(dense) <= lo):
            raise _lib.EffqError("torch.sigmoid(x) >= 0.5 is not monotone around its threshold")
        self._sig_thresh = float(-torch.tensor([lo], dtype=torch.int32).view(torch.float32).item())
        return self._sig_thresh

    @staticmethod
    def _fuse_code(what: str, fuse, argmax: bool, by: str, Cc: int, rule: Optional[str] = None) -> int:
        """The code of the merge type `fuse`, checked for a decision by argmax or by sigmoid (named `by` in the refusal),
        together with the class count and, for the label rule 'brats', its three channels."""
        key = fuse.lower() if isinstance(fuse, str) else fuse
        if key not in _lib.SEG_FUSE or (argmax and key is not None):
            raise _lib.EffqError(f"{what}: merge type {fuse!r} for {by}")
        if not 0 < Cc <= _lib.SEG_TALLIES_MAX_CLASSES:
            raise _lib.EffqError(f"{what}: {Cc} classes, at most {_lib.SEG_TALLIES_MAX_CLASSES}")
        if rule == "brats" and Cc < 3:
            raise _lib.EffqError(f"{what}: the brats rule needs 3 channels or more, got {Cc}")
        return _lib.SEG_FUSE[key]

    def _seg_case(self, what: str, logits: torch.Tensor, label: torch.Tensor, task: str, fuse, spatial: bool):
        """The arguments of one case that seg_tallies, seg_lesions, seg_surface and seg_surface_mm share, checked:
        returns (x, lab, Cc, extents, mode, fuse code, thresh) - the fp32 logits, the contiguous label, the class count,
        (D, H, W) when `spatial` requires C x D x H x W logits and the voxel count S otherwise, and the decision."""
        x = self._f32(logits)
        if spatial and x.dim() != 4:
            raise _lib.EffqError(f"{what}: expected C x D x H x W logits, got {tuple(x.shape)}")
        Cc = int(x.shape[0])
        extents = tuple(int(i) for i in x.shape[1:]) if spatial else x[0].numel()
        mode = _decision_mode(task, ("lits", "brats"), f"Unknown task {task}")
        if mode == _lib.SEG_ARGMAX:
            lshape, thresh = tuple(x.shape[1:]), 0.0
        else:
            lshape, thresh = tuple(x.shape), self.sigmoid_threshold()
        fcode = self._fuse_code(what, fuse, mode == _lib.SEG_ARGMAX, f"task {task}", Cc)
        if tuple(label.shape) != lshape or label.dtype != torch.uint8 or label.device != x.device:
            raise _lib.EffqError(f"{what}: label {tuple(label.shape)} {label.dtype} on {label.device}, "
                                 f"needs {lshape} torch.uint8 on {x.device}")
        return x, label.contiguous(), Cc, extents, mode, fcode, thresh

    def _mask_planes(self, what: str, mask: torch.Tensor):
        """(m, P, D, H, W) of the masks cc_label, edt_sq and edt_sq_mm take: D x H x W or P x D x H x W uint8, not empty,
        on the device of the ops; m is contiguous."""
        if mask.dim() not in (3, 4) or mask.dtype != torch.uint8 or mask.numel() == 0:
            raise _lib.EffqError(f"{what}: mask {tuple(mask.shape)} {mask.dtype}, needs (P x) D x H x W torch.uint8")
        if self._elsewhere(mask):
            raise _lib.EffqError(f"{what}: mask on {mask.device}, ops on {self.device}")
        m = mask.contiguous()
        D, H, W = (int(i) for i in m.shape[-3:])
        return m, (int(m.shape[0]) if m.dim() == 4 else 1), D, H, W

    def seg_tallies(self, logits: torch.Tensor, label: torch.Tensor, task: str, fuse: Optional[str] = None):
        """TP, FP, FN, TN per class (C x 4 int64) of one case's stitched logits (C x D x H x W) against its label
        (effq_seg_tallies): lits = argmax over the channels vs class ids (D x H x W); brats = sigmoid >= 0.5 per channel,
        merged by `fuse` (None / 'agg' / 'con'), vs a C x D x H x W 0/1 label."""
        x, lab, Cc, S, mode, fcode, thresh = self._seg_case("seg_tallies", logits, label, task, fuse, False)
        counts = torch.empty(Cc, 4, dtype=torch.int64, device=self.device)
        ws = self._workspace("seg_tallies", _lib.SEG_TALLIES_WS_BYTES)
        check(self.lib.effq_seg_tallies(_ptr(x), _ptr(lab), Cc, S, mode, fcode, thresh, _ptr(counts), _ptr(ws), ws.numel(),
                                        self.stream), "effq_seg_tallies")
        return counts

    def seg_sweep(self, logits: torch.Tensor, label: torch.Tensor, task: str, fuse: Optional[str] = None):
        """The threshold sweep of one case (effq_seg_sweep), arguments as seg_tallies: C x 2 x 4096 int64 on the device,
        [c][g][b] = the voxels with truth g for class c whose score for class c falls in bin b of sweep_edges.  The
        counts of the decision "score >= edge k" are the sums over the bins from k on; row 2048 is seg_tallies at the
        default threshold, which is the pinned edge whatever set_decision_threshold set."""
        x, lab, Cc, S, mode, fcode, _ = self._seg_case("seg_sweep", logits, label, task, fuse, False)
        if not 0 < S < 2 ** 31:
            raise _lib.EffqError(f"seg_sweep: {S} voxels, needs 1 to 2^31 - 1")
        thresh = 0.0 if mode == _lib.SEG_ARGMAX else self.default_sigmoid_threshold()
        hist = torch.empty(Cc, 2, _lib.SEG_SWEEP_BINS, dtype=torch.int64, device=self.device)
        check(self.lib.effq_seg_sweep(_ptr(x), _ptr(lab), Cc, S, mode, fcode, thresh, _ptr(hist), self.stream),
              "effq_seg_sweep")
        return hist

    def seg_sweep_plan(self, Cc: int, S: int, task: str) -> dict:
        """The launch seg_sweep makes for Cc classes and S voxels (effq_seg_sweep_plan): grid, the workgroups, and trips,
        the trips of each over its groups of four voxels."""
        mode = _decision_mode(task, ("lits", "brats"), f"Unknown task {task}")
        grid, trips = C.c_int(0), C.c_int(0)
        check(self.lib.effq_seg_sweep_plan(int(Cc), int(S), mode, C.byref(grid), C.byref(trips)), "effq_seg_sweep_plan")
        return {"grid": grid.value, "trips": trips.value}

    def sweep_edges(self, kind: str) -> torch.Tensor:
        """The 4096 fp32 edges of seg_sweep's bins on the host (effq_seg_sweep_edges), index 0 = -inf: kind 'lits' /
        'argmax' (edge 2048 = 0) or 'brats' / 'sigmoid' (edge 2048 = the default sigmoid threshold)."""
        mode = _decision_mode(kind, tuple(_DECISION_MODES), f"sweep_edges: unknown kind {kind!r} (argmax or sigmoid)")
        thresh = 0.0 if mode == _lib.SEG_ARGMAX else self.default_sigmoid_threshold()
        edges = (C.c_float * _lib.SEG_SWEEP_BINS)()
        check(self.lib.effq_seg_sweep_edges(mode, thresh, edges), "effq_seg_sweep_edges")
        return torch.frombuffer(bytearray(edges), dtype=torch.float32).clone()

    def seg_labels(self, logits: torch.Tensor, rule: str, fuse: Optional[str] = None, dtype=torch.uint8):
        """Label maps of N cases' logits (N x C x spatial, fp32) from the decisions seg_tallies counts
        (effq_seg_labels).  rule 'argmax': class ids of torch.max (fuse None); 'brats': merge_label_brats of the
        sigmoid >= 0.5 channels merged by `fuse` (0 / 1 / 2 / 4, C >= 3); 'rank': i + 1 of the highest set merged
        channel (fuse 'con': get_pred_brats_con_merge); 'planes': the merged 0/1 channels themselves.  Returns
        N x spatial of `dtype` (torch.uint8 / torch.uint16), or N x C x spatial uint8 for 'planes'."""
        x = self._f32(logits)
        if x.dim() < 3:
            raise _lib.EffqError(f"seg_labels: expected N x C x spatial logits, got {tuple(x.shape)}")
        N, Cc, S = int(x.shape[0]), int(x.shape[1]), math.prod(x.shape[2:])
        fcode = _label_rule("seg_labels", rule, fuse, Cc)
        if dtype not in (torch.uint8, torch.uint16) or (rule == "planes" and dtype != torch.uint8):
            raise _lib.EffqError(f"seg_labels: output {dtype} for rule {rule}")
        if N == 0 or S == 0 or N > 65535:
            raise _lib.EffqError(f"seg_labels: {N} cases of {S} voxels")
        shape = tuple(x.shape) if rule == "planes" else (N,) + tuple(x.shape[2:])
        out = torch.empty(shape, dtype=dtype, device=self.device)
        thresh = 0.0 if rule == "argmax" else self.sigmoid_threshold()
        check(self.lib.effq_seg_labels(_ptr(x), N, Cc, S, _lib.SEG_LABEL_RULES[rule], fcode, thresh,
                                       out.element_size(), _ptr(out), self.stream), "effq_seg_labels")
        return out

    def seg_labels_source(self, logits: torch.Tensor, pmin, grid, factors, source_shape, rule: str,
                          fuse: Optional[str] = None) -> torch.Tensor:
        """The label map of one subject on its SOURCE grid (effq_seg_labels_source): `logits` C x d x h x w fp32 are the
        stitched logits on the box pmin : pmin + (d, h, w) of the working grid `grid`, which prep made from the source
        grid `source_shape` with `factors` = target spacing / source spacing per axis (None: 1, no resampling).  Every
        source voxel whose centre falls into the box gets the label of `rule` ('argmax', 'brats', 'rank'; 'planes' is
        refused) and `fuse` from the trilinearly interpolated logits, every other voxel 0.  Returns uint8 of
        `source_shape`."""
        x = self._f32(logits)
        if x.dim() != 4:
            raise _lib.EffqError(f"seg_labels_source: expected C x d x h x w logits, got {tuple(x.shape)}")
        Cc = int(x.shape[0])
        fcode = _label_rule("seg_labels_source", rule, fuse, Cc)
        geo = _source_grid("seg_labels_source", x, pmin, grid, factors, source_shape, 1,
                           "seg_labels_source: source grid {src}: 1 to 32767 along an axis, 2^31 - 1 voxels at most")
        out = torch.empty(tuple(geo[3]), dtype=torch.uint8, device=self.device)
        thresh = 0.0 if rule == "argmax" else self.sigmoid_threshold()
        check(self.lib.effq_seg_labels_source(_ptr(x), Cc, (C.c_int * 3)(*(int(v) for v in x.shape[1:])), *geo,
                                              _lib.SEG_LABEL_RULES[rule], fcode, thresh, _ptr(out), self.stream),
              "effq_seg_labels_source")
        return out

    def seg_probs_source(self, logits: torch.Tensor, pmin, grid, factors, source_shape, mode: str,
                         want_prob: bool = True, want_unc: bool = False):
        """The probability planes and the uncertainty of one subject on its SOURCE grid (effq_seg_probs_source):
        `logits`, `pmin`, `grid`, `factors` and `source_shape` as seg_labels_source, whose interpolated logits these are
        computed from.  mode 'argmax' (class ids: softmax over the C channels, entropy as a share of ln C) or 'sigmoid'
        (per raw channel; the largest binary entropy in bits).  Returns (probs, unc): C x source and source, uint8 levels
        of 1 / 255, each None when not wanted; outside the box probs are 0 (argmax: channel 0 is 255) and unc is 0."""
        x = self._f32(logits)
        if x.dim() != 4:
            raise _lib.EffqError(f"seg_probs_source: expected C x d x h x w logits, got {tuple(x.shape)}")
        Cc = int(x.shape[0])
        code = _decision_mode(mode, ("argmax", "sigmoid"), f"seg_probs_source: unknown mode {mode!r} (argmax or sigmoid)")
        if not 0 < Cc <= _lib.SEG_TALLIES_MAX_CLASSES:
            raise _lib.EffqError(f"seg_probs_source: {Cc} classes, at most {_lib.SEG_TALLIES_MAX_CLASSES}")
        if not (want_prob or want_unc):
            raise _lib.EffqError("seg_probs_source: neither the probabilities nor the uncertainty is wanted")
        geo = _source_grid("seg_probs_source", x, pmin, grid, factors, source_shape, Cc if want_prob else 1,
                           "seg_probs_source: source grid {src}, {planes} planes: 1 to 32767 along an axis, "
                           "2^31 - 1 bytes at most")
        src = tuple(geo[3])
        probs = torch.empty((Cc,) + src, dtype=torch.uint8, device=self.device) if want_prob else None
        unc = torch.empty(src, dtype=torch.uint8, device=self.device) if want_unc else None
        check(self.lib.effq_seg_probs_source(_ptr(x), Cc, (C.c_int * 3)(*(int(v) for v in x.shape[1:])), *geo, code,
                                             _ptr(probs), _ptr(unc), self.stream), "effq_seg_probs_source")
        return probs, unc

    def seg_agreement(self, logits_q: torch.Tensor, logits_fp: torch.Tensor, mode: str, fuse: Optional[str] = None,
                      want_map: bool = False):
        """Where and how much two networks differ on one case (effq_seg_agreement): the stitched last-head logits of the
        calibrated and of the FP network, C x spatial fp32 each.  mode 'argmax' (or the task 'lits') / 'sigmoid' ('brats')
        and `fuse` as seg_tallies: both networks' voxels are decided by its rule.  Returns (counts, flips, stats, map):
        counts C x 4 int64 = both, Q only, FP only, neither (TP, FP, FN, TN with the FP decision as the truth); flips (1)
        int64, the voxels decided differently in any class; stats C x 4 float64 = sum (q - f)^2, sum f^2, max |q - f|,
        sum |p_q - p_f| (p: sigmoid of the channel / softmax over the channels, in fp64); map: uint8 of the spatial
        shape with bit c set where class c is decided differently, or None without `want_map`."""
        if logits_q.dtype != torch.float32 or logits_fp.dtype != torch.float32:
            raise _lib.EffqError(f"seg_agreement: expected float32 logits, got {logits_q.dtype} and {logits_fp.dtype}")
        if logits_q.shape != logits_fp.shape or logits_q.dim() < 2 or logits_q.numel() == 0:
            raise _lib.EffqError(f"seg_agreement: logits {tuple(logits_q.shape)} and {tuple(logits_fp.shape)}, needs the "
                                 f"same C x spatial shape for both")
        if logits_q.device != logits_fp.device:
            raise _lib.EffqError(f"seg_agreement: logits on {logits_q.device} and on {logits_fp.device}")
        if not (logits_q.is_contiguous() and logits_fp.is_contiguous()):
            raise _lib.EffqError("seg_agreement: the logits must be contiguous")
        q, f = self._f32(logits_q), self._f32(logits_fp)
        Cc, S = int(q.shape[0]), q[0].numel()
        key = _decision_mode(mode, tuple(_DECISION_MODES), f"seg_agreement: unknown mode {mode!r} (argmax or sigmoid)")
        fcode = self._fuse_code("seg_agreement", fuse, key == _lib.SEG_ARGMAX, f"mode {mode}", Cc)
        thresh = 0.0 if key == _lib.SEG_ARGMAX else self.sigmoid_threshold()
        counts = torch.empty(Cc, 4, dtype=torch.int64, device=self.device)
        flips = torch.empty(1, dtype=torch.int64, device=self.device)
        stats = torch.empty(Cc, 4, dtype=torch.float64, device=self.device)
        vmap = torch.empty(tuple(q.shape[1:]), dtype=torch.uint8, device=self.device) if want_map else None
        ws = self._workspace("seg_agreement", _lib.SEG_AGREEMENT_WS_BYTES)
        check(self.lib.effq_seg_agreement(_ptr(q), _ptr(f), Cc, S, key, fcode, thresh, _ptr(counts),
                                          _ptr(flips), _ptr(stats), _ptr(vmap), _ptr(ws), ws.numel(), self.stream),
              "effq_seg_agreement")
        return counts, flips, stats, vmap

    def cc_label(self, mask: torch.Tensor, connectivity: int = 26):
        """Connected components of 0/1 volumes (effq_cc_label; scipy.ndimage.label in metrics.py:69-73): `mask` D x H x W
        or P x D x H x W uint8, non-zero = foreground.  Returns (labels, ncomp): int32 labels of the mask's shape, 0 for
        background and 1 + the least linear index of the voxel's component otherwise, and the int64 component count of
        each mask.  connectivity 26 (3 x 3 x 3 neighbourhood) or 6 (faces)."""
        m, P, D, H, W = self._mask_planes("cc_label", mask)
        _connectivity("cc_label", connectivity)
        _plane_limits("cc_label", m, P, D, H, W)
        labels = torch.empty(m.shape, dtype=torch.int32, device=self.device)
        ncomp = torch.empty(P, dtype=torch.int64, device=self.device)
        ws = self._workspace("cc", self.lib.effq_cc_ws_bytes(P, D, H, W))
        check(self.lib.effq_cc_label(_ptr(m), P, D, H, W, int(connectivity), _ptr(labels), _ptr(ncomp), _ptr(ws),
                                     ws.numel(), self.stream), "effq_cc_label")
        return labels, (ncomp if m.dim() == 4 else ncomp[0])

    def seg_lesions(self, logits: torch.Tensor, label: torch.Tensor, task: str, fuse: Optional[str] = None):
        """The lesion-level columns of one case (C x 4 int64: totall, predl, fnl, fpl - components of the label mask, of
        the predicted mask, label components without a predicted voxel, predicted components without a labelled voxel;
        metrics.py:69-94 with the 3 x 3 x 3 neighbourhood) from its stitched logits (C x D x H x W) and its label
        (effq_seg_lesions).  Arguments and decisions as seg_tallies."""
        x, lab, Cc, (D, H, W), mode, fcode, thresh = self._seg_case("seg_lesions", logits, label, task, fuse, True)
        if D * H * W == 0 or 2 * Cc * D * H * W >= 2 ** 31:
            raise _lib.EffqError(f"seg_lesions: {2 * Cc} masks of {D * H * W} voxels (2^31 - 1 voxels in all at most)")
        counts = torch.empty(Cc, 4, dtype=torch.int64, device=self.device)
        ws = self._workspace("cc", self.lib.effq_cc_ws_bytes(2 * Cc, D, H, W))
        check(self.lib.effq_seg_lesions(_ptr(x), _ptr(lab), Cc, D, H, W, mode, fcode, thresh, _lib.LESION_CONNECTIVITY,
                                        _ptr(counts), _ptr(ws), ws.numel(), self.stream), "effq_seg_lesions")
        return counts

    def _table_call(self, what: str, P: int, head: int, width: int, max_rows, call):
        """The calls of cc_table and seg_lesion_table: one int32 buffer holds `head` int64 words (the counts), the P
        int64 row counts and the P x capacity x width table, so one copy brings all of it to the host.  `call(cap, head
        pointer, nrows pointer, rows pointer)` launches.  A plane with more components than the capacity: once more with
        the capacity the row counts give.  Returns (head int64, nrows int64 (P), [rows of plane p, int32 n_p x width]),
        all on the host."""
        cap = _lib.LESION_TABLE_ROWS if max_rows is None else int(max_rows)
        if cap <= 0:
            raise _lib.EffqError(f"{what}: max_rows {max_rows}, needs a positive capacity")
        while True:
            if P * cap * width >= 2 ** 31:
                raise _lib.EffqError(f"{what}: a table of {P} x {cap} rows")
            front = 2 * (head + P)
            buf = torch.empty(front + P * cap * width, dtype=torch.int32, device=self.device)
            base = buf.data_ptr()
            call(cap, C.c_void_p(base), C.c_void_p(base + 8 * head), C.c_void_p(base + 4 * front))
            host = buf.cpu()
            words = host[:front].view(torch.int64)
            nrows = words[head:]
            most = int(nrows.max())
            if most <= cap:
                table = host[front:].view(P, cap, width)
                return words[:head], nrows, [table[q, :int(nrows[q])] for q in range(P)]
            cap = most

    def cc_table(self, mask: torch.Tensor, connectivity: int = 26, max_rows: Optional[int] = None):
        """One record per connected component of 0/1 volumes (effq_cc_table; scipy.ndimage.label + numpy.bincount):
        `mask` as cc_label.  Returns (rows, nrows) on the host: int32 rows n x 2 = first voxel (linear index), size in
        voxels, in ascending order of the first voxel (row k is scipy's component k + 1) - one tensor for a D x H x W
        mask, a list of P for P x D x H x W - and the int64 component count(s).  max_rows: the rows per mask asked for
        first (default _lib.LESION_TABLE_ROWS); a mask with more components costs one more call, all rows are returned."""
        m, P, D, H, W = self._mask_planes("cc_table", mask)
        _connectivity("cc_table", connectivity)
        _plane_limits("cc_table", m, P, D, H, W)

        def call(cap, _head, nrows, rows):
            ws = self._workspace("cc", self.lib.effq_cc_table_ws_bytes(P, D, H, W, cap))
            check(self.lib.effq_cc_table(_ptr(m), P, D, H, W, int(connectivity), cap, rows, nrows, _ptr(ws), ws.numel(),
                                         self.stream), "effq_cc_table")
        _, nrows, rows = self._table_call("cc_table", P, 0, 2, max_rows, call)
        return (rows, nrows) if m.dim() == 4 else (rows[0], nrows[0])

    def seg_lesion_table(self, logits: torch.Tensor, label: torch.Tensor, task: str, fuse: Optional[str] = None,
                         max_rows: Optional[int] = None):
        """The lesions of one case one by one (effq_seg_lesion_table), arguments and decisions as seg_lesions.  Returns
        (counts, nrows, rows) on the host: counts C x 4 int64, bit for bit seg_lesions'; nrows (2 C) int64, the components
        of plane q - the predicted mask of class q for q < C, the label mask of class q - C otherwise; rows, a list of
        2 C int32 tensors n_q x 3 = first voxel (linear index), size, overlap (the voxels that the other mask of the
        class holds too), in ascending order of the first voxel.  max_rows as cc_table."""
        x, lab, Cc, (D, H, W), mode, fcode, thresh = self._seg_case("seg_lesion_table", logits, label, task, fuse, True)
        if D * H * W == 0 or 2 * Cc * D * H * W >= 2 ** 31:
            raise _lib.EffqError(f"seg_lesion_table: {2 * Cc} masks of {D * H * W} voxels (2^31 - 1 voxels in all at most)")

        def call(cap, counts, nrows, rows):
            ws = self._workspace("cc", self.lib.effq_cc_table_ws_bytes(2 * Cc, D, H, W, cap))
            check(self.lib.effq_seg_lesion_table(_ptr(x), _ptr(lab), Cc, D, H, W, mode, fcode, thresh,
                                                 _lib.LESION_CONNECTIVITY, cap, counts, nrows, rows, _ptr(ws), ws.numel(),
                                                 self.stream), "effq_seg_lesion_table")
        counts, nrows, rows = self._table_call("seg_lesion_table", 2 * Cc, 4 * Cc, 3, max_rows, call)
        return counts.view(Cc, 4), nrows, rows

    def label_clean(self, label_map: torch.Tensor, rules, connectivity: int = 26, out: Optional[torch.Tensor] = None):
        """A predicted label map cleaned by connected components (effq_label_clean, --post): `label_map` D x H x W uint8;
        `rules` a list of at most _lib.LABEL_CLEAN_MAX_RULES (labels, op, n, to) - config.PostRule - applied in order,
        each to the map the previous one left: op 'largest' keeps the largest component of the voxels whose value is one
        of `labels` (of equal sizes the one whose first voxel comes first) and gives every other component the value
        `to`; op 'min' gives `to` to every component of fewer than `n` voxels.  Ops 'fill', 'close' and 'open'
        (effq_label_post, called when a rule has one of them): 'fill' gives `to` to every hole of the mask (a component
        of its complement, at the dual connectivity, that touches no face of the volume), 'close' to the voxels that
        closing by a ball of `n` voxels (1 to _lib.LABEL_POST_MAX_RADIUS) adds - for both `to` is one of `labels` -
        and 'open' to the voxels of the mask that opening by such a ball removes.  connectivity 26 or 6.  Returns (map,
        stats): the cleaned map (a new tensor, or `out`, which may be `label_map` itself) and R x 2 int64 on the device:
        per rule the components its mask had ('fill': the holes filled; 'close', 'open': the voxels of the mask before
        the rule) and the voxels it relabelled."""
        m, P, D, H, W = self._mask_planes("label_clean", label_map)
        if m.dim() != 3:
            raise _lib.EffqError(f"label_clean: map {tuple(m.shape)}, needs D x H x W")
        _connectivity("label_clean", connectivity)
        if m.numel() >= 2 ** 31:
            raise _lib.EffqError(f"label_clean: a map of {m.numel()} voxels (2^31 - 1 at most)")
        rules = list(rules)
        R = len(rules)
        if not 1 <= R <= _lib.LABEL_CLEAN_MAX_RULES:
            raise _lib.EffqError(f"label_clean: {R} rules, 1 to {_lib.LABEL_CLEAN_MAX_RULES}")
        sets = (C.c_uint8 * (256 * R))()
        words = (C.c_longlong * (3 * R))()
        morph, max_radius = False, 0
        for r, rule in enumerate(rules):
            try:
                labels, op, n, to = rule
                labels, n, to = [int(v) for v in labels], int(n), int(to)
            except (TypeError, ValueError) as e:
                raise _lib.EffqError(f"label_clean: rule {r}: {rule!r} is no (labels, op, n, to): {e}") from e
            if op not in _lib.LABEL_CLEAN_OPS and op not in _lib.LABEL_POST_OPS:
                raise _lib.EffqError(f"label_clean: rule {r}: unknown op {op!r} (one of "
                                     f"{', '.join(list(_lib.LABEL_CLEAN_OPS) + list(_lib.LABEL_POST_OPS))})")
            if not labels or min(labels) < 1 or max(labels) > 255:
                raise _lib.EffqError(f"label_clean: rule {r}: labels {labels}, needs values of 1 to 255")
            if op in ("fill", "close"):
                if to not in labels:
                    raise _lib.EffqError(f"label_clean: rule {r}: {op} adds voxels to the mask: the new label {to} is "
                                         f"not one of {labels}")
            elif not 0 <= to <= 255 or to in labels:
                raise _lib.EffqError(f"label_clean: rule {r}: the new label {to} is outside 0..255 or one of {labels}")
            if op == "min" and n < 1:
                raise _lib.EffqError(f"label_clean: rule {r}: min {n}, needs 1 or more voxels")
            if op in ("close", "open"):
                if not 1 <= n <= _lib.LABEL_POST_MAX_RADIUS:
                    raise _lib.EffqError(f"label_clean: rule {r}: {op} {n}, needs a radius of 1 to "
                                         f"{_lib.LABEL_POST_MAX_RADIUS} voxels")
                max_radius = max(max_radius, n)
            for v in labels:
                sets[256 * r + v] = 1
            code = _lib.LABEL_CLEAN_OPS[op] if op in _lib.LABEL_CLEAN_OPS else _lib.LABEL_POST_OPS[op]
            words[3 * r], words[3 * r + 1], words[3 * r + 2] = code, n, to
            morph = morph or op in _lib.LABEL_POST_OPS
        if out is None:
            out = torch.empty_like(m)
        elif out.shape != m.shape or out.dtype != torch.uint8 or out.device != m.device or not out.is_contiguous():
            raise _lib.EffqError(f"label_clean: out {tuple(out.shape)} {out.dtype} on {out.device}, needs a contiguous "
                                 f"{tuple(m.shape)} torch.uint8 on {m.device}")
        elif out is label_map and m is not label_map:
            raise _lib.EffqError("label_clean: a map cleaned in place must be contiguous")
        stats = torch.empty(R, 2, dtype=torch.int64, device=self.device)
        if not morph:
            ws = self._workspace("label_clean", self.lib.effq_label_clean_ws_bytes(D, H, W))
            check(self.lib.effq_label_clean(_ptr(m), D, H, W, int(connectivity), R, sets, words, _ptr(out), _ptr(stats),
                                            _ptr(ws), ws.numel(), self.stream), "effq_label_clean")
            return out, stats
        need = self.lib.effq_label_post_ws_bytes(D, H, W, max_radius)
        if need == 0:
            raise _lib.EffqError(f"label_clean: a map {D} x {H} x {W} padded by the radius {max_radius} is outside the "
                                 f"distance transform's limits (fewer than 2^31 voxels, D and H at most "
                                 f"{_lib.EDT_MAX_LINE})")
        ws = self._workspace("label_clean", need)
        check(self.lib.effq_label_post(_ptr(m), D, H, W, int(connectivity), R, sets, words, _ptr(out), _ptr(stats),
                                       _ptr(ws), ws.numel(), self.stream), "effq_label_post")
        return out, stats

    def label_tallies(self, pred: torch.Tensor, truth: torch.Tensor, lut, C_: int):
        """TP, FP, FN, TN per class (C x 4 int64, seg_tallies' layout) of a uint8 label map against the truth
        (effq_label_tallies).  `lut`: 256 integers, bit c set = that label value belongs to class c; `truth`: a label map
        of `pred`'s shape, read through `lut`, or C 0/1 planes (C x pred's shape)."""
        Cc = int(C_)
        if pred.dtype != torch.uint8 or truth.dtype != torch.uint8 or pred.numel() == 0:
            raise _lib.EffqError(f"label_tallies: pred {tuple(pred.shape)} {pred.dtype}, truth {tuple(truth.shape)} "
                                 f"{truth.dtype}: needs torch.uint8, not empty")
        if not 0 < Cc <= _lib.SEG_TALLIES_MAX_CLASSES:
            raise _lib.EffqError(f"label_tallies: {Cc} classes, at most {_lib.SEG_TALLIES_MAX_CLASSES}")
        if tuple(truth.shape) == tuple(pred.shape):
            planes = 0
        elif tuple(truth.shape) == (Cc,) + tuple(pred.shape):
            planes = 1
        else:
            raise _lib.EffqError(f"label_tallies: truth {tuple(truth.shape)} for a map {tuple(pred.shape)}: needs the "
                                 f"map's shape, or {Cc} planes of it")
        for t, who in ((pred, "pred"), (truth, "truth")):
            if self._elsewhere(t):
                raise _lib.EffqError(f"label_tallies: {who} on {t.device}, ops on {self.device}")
        try:
            table = [int(v) for v in lut]
        except (TypeError, ValueError) as e:
            raise _lib.EffqError(f"label_tallies: lut: {e}") from e
        if len(table) != 256 or min(table) < 0 or max(table) >= 1 << Cc:
            raise _lib.EffqError(f"label_tallies: lut of {len(table)} entries, needs 256 of {Cc} class bits each")
        p, t = pred.contiguous(), truth.contiguous()
        counts = torch.empty(Cc, 4, dtype=torch.int64, device=self.device)
        ws = self._workspace("label_tallies", self.lib.effq_label_tallies_ws_bytes())
        check(self.lib.effq_label_tallies(_ptr(p), _ptr(t), planes, Cc, p.numel(), (C.c_uint16 * 256)(*table),
                                          _ptr(counts), _ptr(ws), ws.numel(), self.stream), "effq_label_tallies")
        return counts

    def edt_sq(self, mask: torch.Tensor):
        """Exact squared Euclidean distance transform (effq_edt_sq): `mask` D x H x W or P x D x H x W uint8, non-zero =
        site.  Returns an int32 tensor of the mask's shape: the squared distance (voxel units) of every voxel to the
        nearest site of its own volume, 0 on a site, INT32_MAX throughout a volume without sites.  It is
        rint(scipy.ndimage.distance_transform_edt(mask == 0) ** 2), voxel for voxel."""
        m, P, D, H, W = self._mask_planes("edt_sq", mask)
        need = self.lib.effq_surf_ws_bytes(P, D, H, W)
        if need == 0:
            raise _lib.EffqError(f"edt_sq: {P} masks of {D} x {H} x {W} voxels (at most 65535 masks, 2^31 - 1 voxels in "
                                 f"all, D^2 + H^2 + W^2 < 2^31, D and H at most {_lib.EDT_MAX_LINE})")
        sq = torch.empty(m.shape, dtype=torch.int32, device=self.device)
        ws = self._workspace("surf", need)
        check(self.lib.effq_edt_sq(_ptr(m), P, D, H, W, _ptr(sq), _ptr(ws), ws.numel(), self.stream), "effq_edt_sq")
        return sq

    def seg_surface(self, logits: torch.Tensor, label: torch.Tensor, task: str, fuse: Optional[str] = None):
        """What the surface distances of one case need (effq_seg_surface), from its stitched logits (C x D x H x W) and
        its label, arguments and decisions as seg_tallies.  Returns (counts, sums): counts C x 6 int64 = nP, nL,
        maxsq_PL, maxsq_LP, qlo_sq, qhi_sq and sums C x 2 float64 = the sums of the directed distances
        (include/effq_hip.h); evaluate.surface_metrics turns them into hd, hd95 and assd."""
        x, lab, Cc, (D, H, W), mode, fcode, thresh = self._seg_case("seg_surface", logits, label, task, fuse, True)
        need = self.lib.effq_surf_ws_bytes(2 * Cc, D, H, W) if D * H * W else 0
        if need == 0:
            raise _lib.EffqError(f"seg_surface: {2 * Cc} masks of {D} x {H} x {W} voxels (2^31 - 1 voxels in all at "
                                 f"most, D^2 + H^2 + W^2 < 2^31, D and H at most {_lib.EDT_MAX_LINE})")
        counts = torch.empty(Cc, 6, dtype=torch.int64, device=self.device)
        sums = torch.empty(Cc, 2, dtype=torch.float64, device=self.device)
        ws = self._workspace("surf", need)
        check(self.lib.effq_seg_surface(_ptr(x), _ptr(lab), Cc, D, H, W, mode, fcode, thresh, _ptr(counts), _ptr(sums),
                                        _ptr(ws), ws.numel(), self.stream), "effq_seg_surface")
        return counts, sums

    @staticmethod
    def _axis_weights(what: str, spacing):
        """The fp32 weights of the three axes, float32(float64(spacing) ** 2), from a spacing of three finite positive
        numbers (millimetres per voxel along D, H, W)."""
        try:
            sp = [float(v) for v in spacing]
        except (TypeError, ValueError):
            sp = []
        if len(sp) != 3 or not all(math.isfinite(v) and v > 0 for v in sp):
            raise _lib.EffqError(f"{what}: spacing {spacing!r}, needs three finite positive numbers (d, h, w)")
        w = [float(np.float32(np.float64(v) ** 2)) for v in sp]
        if not all(math.isfinite(v) and v > 0 for v in w):
            raise _lib.EffqError(f"{what}: the square of spacing {spacing!r} is not a positive finite float32")
        return w

    def edt_sq_mm(self, mask: torch.Tensor, spacing):
        """Squared Euclidean distance transform on a grid of spacing (d, h, w) (effq_edt_sq_mm): `mask` D x H x W or
        P x D x H x W uint8, non-zero = site.  Returns a float32 tensor of the mask's shape: for every voxel the least
        fl(fl(fl(ww dw^2) + fl(wh dh^2)) + fl(wd dd^2)) over the sites of its own volume, wa = float32(spacing_a ** 2) -
        the bits of the brute force in fp32 -, 0 on a site, +inf throughout a volume without sites."""
        m, P, D, H, W = self._mask_planes("edt_sq_mm", mask)
        wd, wh, ww = self._axis_weights("edt_sq_mm", spacing)
        need = self.lib.effq_surf_mm_ws_bytes(P, D, H, W)
        if need == 0:
            raise _lib.EffqError(f"edt_sq_mm: {P} masks of {D} x {H} x {W} voxels (at most 65535 masks, 2^31 - 1 voxels "
                                 f"in all, every extent at most {_lib.EDT_MM_MAX_EXTENT})")
        sq = torch.empty(m.shape, dtype=torch.float32, device=self.device)
        ws = self._workspace("surf_mm", need)
        check(self.lib.effq_edt_sq_mm(_ptr(m), P, D, H, W, wd, wh, ww, _ptr(sq), _ptr(ws), ws.numel(), self.stream),
              "effq_edt_sq_mm")
        return sq

    def seg_surface_mm(self, logits: torch.Tensor, label: torch.Tensor, task: str, fuse: Optional[str] = None,
                       spacing=(1.0, 1.0, 1.0)):
        """What the surface distances of one case in millimetres need (effq_seg_surface_mm), from its stitched logits
        (C x D x H x W), its label and the spacing (d, h, w) of its grid; arguments and decisions as seg_surface.
        Returns (counts, sq, sums): counts C x 2 int64 = nP, nL, sq C x 4 float32 = max_PL, max_LP, qlo, qhi (squared
        distances in mm^2) and sums C x 2 float64 = the sums of the directed distances in mm (include/effq_hip.h);
        evaluate.surface_metrics_mm turns them into hd, hd95 and assd."""
        case = self._seg_case("seg_surface_mm", logits, label, task, fuse, True)
        x, lab, Cc, (D, H, W), mode, fcode, thresh = case
        wd, wh, ww = self._axis_weights("seg_surface_mm", spacing)
        need = self.lib.effq_surf_mm_ws_bytes(2 * Cc, D, H, W) if D * H * W else 0
        if need == 0:
            raise _lib.EffqError(f"seg_surface_mm: {2 * Cc} masks of {D} x {H} x {W} voxels (2^31 - 1 voxels in all at "
                                 f"most, every extent at most {_lib.EDT_MM_MAX_EXTENT})")
        counts = torch.empty(Cc, 2, dtype=torch.int64, device=self.device)
        sq = torch.empty(Cc, 4, dtype=torch.float32, device=self.device)
        sums = torch.empty(Cc, 2, dtype=torch.float64, device=self.device)
        ws = self._workspace("surf_mm", need)
        check(self.lib.effq_seg_surface_mm(_ptr(x), _ptr(lab), Cc, D, H, W, mode, fcode, thresh, wd, wh, ww, _ptr(counts),
                                           _ptr(sq), _ptr(sums), _ptr(ws), ws.numel(), self.stream), "effq_seg_surface_mm")
        return counts, sq, sums
