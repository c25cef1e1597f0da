"""Tensor-level front end of the C-ABI library: torch tensors supply device memory and
the HIP stream; every computation is a call into ``libeffq_hip.so``.

No CPU fallback exists here on purpose: tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import Geom, check

ADMM_TOL = 1e-5   # layer_helper.py:55
# tensors from this size on are fitted by the bracketed fixed point (effq_fp_bracket_*)
FP_BRACKET_MIN = 1 << 18
# data-parallel activation fit: after DP_GATHER_AFTER all-reduced iterations the ranks exchange their tallies and undecided
# lists once and finish on their own (effq_fp_bracket_export / _import); lists longer than DP_GATHER_MAX_BYTES in all: more
# all-reduced iterations first
DP_GATHER_AFTER = 4
DP_GATHER_MAX_BYTES = 128 << 20


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def to_ndhwc(x: torch.Tensor) -> torch.Tensor:
    """(N,C,D,H,W) logical -> contiguous (N,D,H,W,C) storage (no copy if already channels_last_3d)."""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def from_ndhwc(t: torch.Tensor) -> torch.Tensor:
    """contiguous (N,D,H,W,C) -> logical (N,C,D,H,W) view (channels_last_3d strides)."""
    return t.permute(0, 4, 1, 2, 3)


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(i) for i in v)


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
    import numpy as np
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


def make_geom(x_shape_ncdhw, c2: int, ksize, stride, padding) -> Geom:
    n, c1, d, h, w = (int(i) for i in x_shape_ncdhw)
    k, s, p = _triple(ksize), _triple(stride), _triple(padding)
    return Geom(n, c1, int(c2), d, h, w, k[0], k[1], k[2], s[0], s[1], s[2], p[0], p[1], p[2])


def _check_shapes(geom: Geom, x, w=None, bias=None, y=None, att=None):
    """Host-side guard: buffer sizes must match what the kernels index (an out-of-bounds access
    on the device can take the whole node down)."""
    od, oh, ow = geom.out_dims()
    if min(od, oh, ow) <= 0:
        raise _lib.EffqError(f"empty conv output for geometry {[getattr(geom, f[0]) for f in geom._fields_]}")
    want = {"x": (x, geom.N * geom.D * geom.H * geom.W * geom.C1),
            "weight": (w, geom.C2 * geom.C1 * geom.KD * geom.KH * geom.KW),
            "bias": (bias, geom.C2),
            "y": (y, geom.N * od * oh * ow * geom.C2),
            "att": (att, geom.N * od * oh * ow)}
    for name, (t, n) in want.items():
        if t is not None and t.numel() != n:
            raise _lib.EffqError(f"{name} has {t.numel()} elements, geometry needs {n}")


CONV_KINDS = ("tiled", "k_conv3d_c4h", "k_conv1_mfma", "k_conv3d_c1h", "k_conv3d_c4")
CONV_I8_KERNELS = (None, "l2e", "l2", "i8<2>", "i8w", "i8g<4>", "i8g<8>", "i8g2<16>")


def conv_plan_query(lib, geom: Geom, loss_only: bool = False) -> dict:
    """The launch conv3d_quant_calib_step makes for a geometry; loss_only: targets, no output, no mask, no fused quantiser
    (effq_conv_plan_query: answered on the host, needs no device).  A refused geometry raises EffqError."""
    out = [C.c_int() for _ in range(8)]
    lds = C.c_longlong()
    check(lib.effq_conv_plan_query(C.byref(geom), int(bool(loss_only)), *[C.byref(o) for o in out], C.byref(lds)),
          "effq_conv_plan_query")
    d = dict(zip(("kind", "fast", "cslab", "nslab", "nt", "grid_x", "grid_y", "ntiles"), (o.value for o in out)))
    d.update(fast=bool(d["fast"]), lds_bytes=lds.value, kernel=CONV_KINDS[d["kind"]])
    return d


def conv_i8_plan_query(lib, geom: Geom, want_out: bool = False) -> dict:
    """The launch conv3d_calib_step_i8 (want_out: conv3d_quant_forward_i8) makes for a geometry (effq_conv_i8_plan_query,
    on the host)."""
    out = [C.c_int() for _ in range(4)]
    check(lib.effq_conv_i8_plan_query(C.byref(geom), int(bool(want_out)), *[C.byref(o) for o in out]),
          "effq_conv_i8_plan_query")
    d = dict(zip(("kind", "grid_x", "grid_y", "ntiles"), (o.value for o in out)))
    d["kernel"] = CONV_I8_KERNELS[d["kind"]]
    return d


def conv_i8s_plan_query(lib, geom: Geom, act_levels: int, w_levels: int) -> dict:
    """The launch conv3d_calib_step_i8s makes for a geometry and a level pair (effq_conv_i8s_plan_query, on the host)."""
    out = [C.c_int() for _ in range(7)]
    check(lib.effq_conv_i8s_plan_query(C.byref(geom), int(act_levels), int(w_levels), *[C.byref(o) for o in out]),
          "effq_conv_i8s_plan_query")
    return dict(zip(("NJ", "CT", "T", "K", "aoff", "wmul", "grid"), (o.value for o in out)))


class HipOps:
    """Per-device handle: stream + library-owned workspaces (grown on demand, never shrunk)."""

    def __init__(self, device: torch.device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.EffqError(f"efficientq_amd runs on a HIP device only, got {device} (no CPU fallback)")
        self.lib = _lib.load()
        self.device = device
        self._red_ws = torch.zeros(self.lib.effq_reduce_ws_bytes(), dtype=torch.uint8, device=device)
        self._ws = {}
        self._att_cache = {}
        self._ws_retired = []

    # -- plumbing ---------------------------------------------------------------------------
    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def loss_stream(self):
        """The stream the per-iteration loss evaluation runs on, one iteration behind the ADMM chain."""
        if getattr(self, "_loss", None) is None:
            self._loss = torch.cuda.Stream(self.device)
        return self._loss

    def side_stream(self):
        """A second HIP stream of this device for work that is independent of the calibration stream."""
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def side_stream2(self):
        """A third stream: the later inverses of a layer alternate between the two side streams."""
        if getattr(self, "_side2", None) is None:
            self._side2 = torch.cuda.Stream(self.device)
        return self._side2

    def warm_streams(self):
        """Create every stream the calibration uses NOW, in a fixed order: HIP hands out hardware queues in creation order
        (4 by default), and streams that share one run their kernels one after the other.  Created lazily - after a
        communicator had brought its own streams - the two side streams of the inverses landed on one queue (the later
        inverses of the 256-channel layers 44 / 63 ms instead of 28 / 32, +5 % per calibration with a 1-rank RCCL group);
        rccl.DirectComm calls this before ncclCommInitRank."""
        if getattr(self, "_warm", False):
            return
        main = torch.cuda.current_stream(self.device)
        # which streams get their helper, in which order, is empirical (per calibration with a 1-rank RCCL group, one box: none
        # 693 ms, main / loss / side / side2 675, main / side / side2 - the order of a run without a communicator - 691; plain
        # run 657; GPU_MAX_HW_QUEUES = 6 / 8: 766 / 753)
        for st in (main, self.loss_stream(), self.side_stream(), self.side_stream2()):
            check(self.lib.effq_spd_inverse_prepare(st.cuda_stream), "effq_spd_inverse_prepare")
        self._warm = True

    def _workspace(self, key: str, nbytes: int) -> torch.Tensor:
        """Library workspace `key`, zero-filled on the current stream when (re)allocated.  A replaced buffer stays
        referenced until release_retired() (kernels of another stream may still be reading it, and the caching
        allocator only orders a block against the stream it was allocated on)."""
        cur = self._ws.get(key)
        if cur is None or cur.numel() < nbytes:
            if cur is not None:
                self._ws_retired.append(cur)
            cur = torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device)
            self._ws[key] = cur
        return cur

    def release_retired(self):
        """Drop replaced workspaces; call only where every stream of this handle has been joined."""
        self._ws_retired.clear()

    def _elsewhere(self, t: torch.Tensor) -> bool:
        return t.device != self.device and not (t.device.type == "cuda" and self.device.index in (None, t.device.index))

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        if self._elsewhere(t):
            raise _lib.EffqError(f"tensor on {t.device}, ops on {self.device}")
        if t.dtype != torch.float32:
            raise _lib.EffqError(f"expected float32, got {t.dtype}")
        return t if t.is_contiguous() else t.contiguous()

    # -- a1/a3 --------------------------------------------------------------------------------
    def quant_dequant_f32(self, x: torch.Tensor, alpha: torch.Tensor, levels: int, lo: float, hi: float,
                          want_idx: bool = False):
        """PTQConv._quantize_act / discretize in fp32 (PTQConv.py:114-116).  alpha: 0-dim device tensor."""
        x = self._f32(x)
        a = self._f32(alpha.reshape(1))
        y = torch.empty_like(x)
        idx = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_idx else None
        check(self.lib.effq_quant_dequant_f32(_ptr(x), _ptr(a), lo, hi, levels, _ptr(y), _ptr(idx), x.numel(),
                                              self.stream), "effq_quant_dequant_f32")
        return (y, idx) if want_idx else y

    def quant_dequant_f64path(self, x: torch.Tensor, state: torch.Tensor, levels: int, lo: float, hi: float,
                              want_b: bool = False, want_idx: bool = False):
        """a*b of project_by_iter (layer_helper.py:66, EfficientQConv.py:70); alpha = state[0] (device double)."""
        x = self._f32(x)
        y = torch.empty_like(x)
        b = torch.empty_like(x) if want_b else None
        idx = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_idx else None
        check(self.lib.effq_quant_dequant_f64path(_ptr(x), _ptr(state), lo, hi, levels, _ptr(y), _ptr(b), _ptr(idx),
                                                  x.numel(), self.stream), "effq_quant_dequant_f64path")
        return y, b, idx

    # -- a2 -----------------------------------------------------------------------------------
    def abs_sum(self, x: torch.Tensor) -> torch.Tensor:
        x = self._f32(x)
        out = torch.empty(2, dtype=torch.float64, device=x.device)
        check(self.lib.effq_abs_sum_f64(_ptr(x), x.numel(), _ptr(out), _ptr(self._red_ws), self.stream),
              "effq_abs_sum_f64")
        return out

    def moments(self, x: torch.Tensor) -> torch.Tensor:
        """[sum, sum of squares, count] in fp64 on the device."""
        x = self._f32(x)
        out = torch.empty(3, dtype=torch.float64, device=x.device)
        check(self.lib.effq_moments_f64(_ptr(x), x.numel(), _ptr(out), _ptr(self._red_ws), self.stream),
              "effq_moments_f64")
        return out

    def new_fp_state(self) -> torch.Tensor:
        # effq_fp_state viewed as 5 doubles: alpha, alpha_prev, sums[2], {iters,done}
        return torch.zeros(5, dtype=torch.float64, device=self.device)

    @staticmethod
    def read_fp_state(state: torch.Tensor):
        host = state.cpu()
        iters, done = host[4:5].view(torch.int32).tolist()
        return float(host[0]), int(iters), int(done)

    def fit_scale(self, x: torch.Tensor, levels: int, lo: float, hi: float, reducer=None,
                  guess_iters: int = 16, state: Optional[torch.Tensor] = None, abs_sums: Optional[torch.Tensor] = None):
        """project_by_iter on the device (layer_helper.py:40-70).

        ``reducer`` (callable on a device fp64 tensor, in place) sums statistics over data-parallel
        ranks; with it the statistics of every iteration are all-reduced before the update.
        Returns (alpha: float, iters: int, state tensor).  Raises RuntimeWarning like the
        reference when the cap 100*L is hit.
        """
        x = self._f32(x)
        n = x.numel()
        st = state if state is not None else self.new_fp_state()
        cap = 100 * levels
        if abs_sums is not None:
            s0 = abs_sums                      # [sum|x|, n], already summed over the data-parallel ranks by the caller
        else:
            s0 = self.abs_sum(x)
            if reducer is not None:
                reducer(s0)
        batch = max(4, int(guess_iters))
        if n >= FP_BRACKET_MIN and levels <= 256:
            return self._fit_scale_bracket(x, n, levels, lo, hi, reducer, batch, st, s0, cap)
        check(self.lib.effq_fp_init(_ptr(st), _ptr(s0), self.stream), "effq_fp_init")
        while True:
            if reducer is None:
                check(self.lib.effq_alpha_fixed_point(_ptr(x), n, levels, lo, hi, ADMM_TOL, cap, batch, _ptr(st),
                                                      _ptr(self._red_ws), self.stream), "effq_alpha_fixed_point")
            else:
                sums = st[2:4]
                done = st[4:5]
                for _ in range(batch):
                    check(self.lib.effq_alpha_stats_f64(_ptr(x), _ptr(st), lo, hi, levels, n, _ptr(sums),
                                                        C.c_void_p(done.data_ptr() + 4), _ptr(self._red_ws),
                                                        self.stream), "effq_alpha_stats_f64")
                    reducer(sums)
                    check(self.lib.effq_fp_update(_ptr(st), ADMM_TOL, cap, self.stream), "effq_fp_update")
            alpha, iters, done = self.read_fp_state(st)   # one host sync per batch
            if done == 1:
                return alpha, iters, st
            if done == 2:
                raise RuntimeWarning(f"Exceed maximum iteration ({cap}) for alpha optimization")
            batch = min(max(8, iters // 2), 256)

    def _fit_scale_bracket(self, x, n, levels, lo, hi, reducer, batch, st, s0, cap):
        """fit_scale on a large tensor by the bracketed fixed point (effq_fp_bracket_*): after the first iterations only
        the values whose level can still change are read.  Same iterates as the per-iteration passes."""
        ws = self._workspace("fp_bracket", self.lib.effq_fp_bracket_ws_bytes(n))
        # unsigned quantiser = post-ReLU input: the first pass already drops the exact zeros
        check(self.lib.effq_fp_bracket_init(_ptr(st), _ptr(s0), n, levels, int(lo == 0.0), _ptr(ws), ws.numel(),
                                            self.stream), "effq_fp_bracket_init")
        gather = (reducer is not None and lo == 0.0 and hasattr(reducer, "all_gather"))
        dp_iters = DP_GATHER_AFTER
        while True:
            if reducer is None:
                check(self.lib.effq_fp_bracket_run(_ptr(x), n, levels, lo, hi, ADMM_TOL, cap, batch, _ptr(st), _ptr(ws),
                                                   self.stream), "effq_fp_bracket_run")
            else:
                sums = st[2:4]
                for _ in range(dp_iters if gather else batch):
                    check(self.lib.effq_fp_bracket_stats(_ptr(x), n, levels, lo, hi, _ptr(st), _ptr(ws), self.stream),
                          "effq_fp_bracket_stats")
                    reducer(sums)
                    check(self.lib.effq_fp_bracket_update(n, levels, lo, hi, ADMM_TOL, cap, _ptr(st), _ptr(ws),
                                                          self.stream), "effq_fp_bracket_update")
                if gather:
                    r = self._fit_scale_gathered(x, n, levels, lo, hi, reducer, st, ws, cap)
                    if not isinstance(r, int):
                        return r
                    dp_iters = r                   # not usable yet (or the gathered fit left its bracket): more all-reduced
                    continue                       # iterations first
            alpha, iters, done = self.read_fp_state(st)   # one host sync per batch
            if done == 1:
                return alpha, iters, st
            if done == 2:
                raise RuntimeWarning(f"Exceed maximum iteration ({cap}) for alpha optimization")
            batch = min(max(8, iters // 2), 256)

    def _fit_scale_gathered(self, x, n, levels, lo, hi, reducer, st, ws, cap):
        """Data-parallel ranks, "gather once" (effq_fp_bracket_export / _import): what is left of every rank's shard under
        the current bracket - four integer tallies and the list of the undecided values - is exchanged with TWO collectives
        (tallies + list lengths + brackets in one all-reduce, the zero-padded lists in one all-gather of a fixed size), and
        every rank finishes the fit on its own, bit-identically.  No host round trip on the way: whether the exchange was
        usable is decided on the device.  Returns (alpha, iters, state), or - when the fit must go on with all-reduced
        iterations: no list yet / lists too long / horizon bracket / an iterate left the bracket of the import - the number of
        such iterations to run before the next attempt."""
        world, rank = reducer.world, reducer.rank
        dev = self.device
        slot = max(4096, min((n + 3) // 4 * 4, DP_GATHER_MAX_BYTES // 4 // max(1, world)))      # floats per rank
        lst = self._workspace("fp_gather_list", 4 * slot).view(torch.float32)
        exp = torch.empty(self.lib.effq_fp_bracket_export_words(), dtype=torch.int64, device=dev)
        check(self.lib.effq_fp_bracket_export(_ptr(ws), n, _ptr(exp), _ptr(lst), slot, self.stream),
              "effq_fp_bracket_export")
        # one int64 message: [0..3] tallies (summed), then one slot triple per rank - list length, bit patterns of the
        # bracket its tallies are valid under (the other ranks add zeros)
        pack = torch.zeros(4 + 3 * world, dtype=torch.int64, device=dev)
        pack[:4] = exp[:4]
        pack[4 + 3 * rank: 7 + 3 * rank] = exp[4:7]
        reducer(pack)
        gathered = reducer.all_gather(lst[:slot])               # second (and last) message of the fit
        m = world * slot
        ws2 = self._workspace("fp_bracket_gathered", self.lib.effq_fp_bracket_ws_bytes(m))
        check(self.lib.effq_fp_bracket_import(_ptr(ws), n, _ptr(pack), world, slot, _ptr(st), _ptr(ws2), ws2.numel(),
                                              self.stream), "effq_fp_bracket_import")
        batch = 12 * levels
        while True:
            check(self.lib.effq_fp_bracket_run(_ptr(gathered), m, levels, lo, hi, ADMM_TOL, cap, batch, _ptr(st), _ptr(ws2),
                                               self.stream), "effq_fp_bracket_run")
            alpha, iters, done = self.read_fp_state(st)         # the fit's one host read (in the common case)
            if done == 1:
                return alpha, iters, st
            if done == 2:
                raise RuntimeWarning(f"Exceed maximum iteration ({cap}) for alpha optimization")
            if done == 4:                                       # exchange not usable / left the bracket of the import:
                check(self.lib.effq_fp_bracket_rebase(_ptr(st), _ptr(ws), n, self.stream), "effq_fp_bracket_rebase")
                # on with all-reduced iterations, from the base - as many as the lists need to shrink into their slots (the
                # undecided share falls by ~0.57 every two iterations at few levels: profiles/r03_fp_bracket_trace_*)
                lens = pack[4::3].cpu().tolist()
                worst = max(lens) if min(lens) >= 0 else 0
                return DP_GATHER_AFTER if worst <= slot else max(2, min(32, int(math.ceil(3.6 * math.log(worst / slot))) + 1))
            batch = min(2 * batch, 256)

    def fp_bracket_diagnostics(self):
        """The header of the bracketed fixed point's workspace after a fit (tests, tuning)."""
        ws = self._ws["fp_bracket"]
        f = ws[:256].view(torch.float64).cpu()
        i = ws[:256].view(torch.int64).cpu()
        return {"blo": float(f[0]), "bhi": float(f[1]), "src": int(i[7]), "G": int(i[10]), "per": int(i[11]),
                "escapes": int(i[12]), "narrowings": int(i[13]), "visited": int(i[14]), "list_total": int(i[15]),
                "density": float(f[17]), "widen": int(i[20]), "base": int(i[21]), "z_total": int(i[22])}

    def weight_fixed_point(self, wstar, dual, v, levels: int, state, guess: int = 16):
        """Projection input v = wstar + dual and its scale fixed point (EfficientQConv.py:108).
        Small tensors: ONE launch, no host round trip (returns None).  Large ones: fused iterations in
        batches with one 40-byte read per batch (returns the iteration count)."""
        n = wstar.numel()
        if n <= self.lib.effq_fp_small_max():
            check(self.lib.effq_fixed_point_small(_ptr(wstar), _ptr(dual), _ptr(v), n, levels, -1.0, 1.0, ADMM_TOL,
                                                  100 * levels, _ptr(state), self.stream), "effq_fixed_point_small")
            return None
        if n <= self.lib.effq_fp_coop_max():
            check(self.lib.effq_fixed_point_coop(_ptr(wstar), _ptr(dual), _ptr(v), n, levels, -1.0, 1.0, ADMM_TOL,
                                                 100 * levels, _ptr(state), _ptr(self._red_ws), self.stream),
                  "effq_fixed_point_coop")
            return None
        self.admm_presum(wstar, dual, v)
        _, it, _ = self.fit_scale(v, levels, -1.0, 1.0, guess_iters=guess, state=state)
        return it

    def fixed_point_bucket(self, a, b, v, levels: int, state, lo: float = -1.0, hi: float = 1.0):
        """project_by_iter of v = a + b (b may be None) on the bucketed copy: one workgroup, one launch
        (effq_fixed_point_bucket)."""
        n = a.numel()
        ws = self._workspace("fp_bucket", self.lib.effq_fp_bucket_ws_bytes(n))
        check(self.lib.effq_fixed_point_bucket(_ptr(a), _ptr(b), _ptr(v), n, levels, lo, hi, ADMM_TOL, 100 * levels,
                                               _ptr(state), _ptr(ws), ws.numel(), self.stream),
              "effq_fixed_point_bucket")

    def new_fp_pred(self) -> torch.Tensor:
        """Zero-filled prediction state of effq_fixed_point_traj (nothing known)."""
        return torch.zeros(self.lib.effq_fp_traj_pred_bytes(), dtype=torch.uint8, device=self.device)

    def fixed_point_traj(self, a, b, v, levels: int, state, pred, lo: float = -1.0, hi: float = 1.0):
        """project_by_iter of v = a + b from the previous call's iterates (`pred`), one launch (effq_fixed_point_traj)."""
        n = a.numel()
        ws = self._workspace("fp_traj", self.lib.effq_fp_traj_ws_bytes(n))
        check(self.lib.effq_fixed_point_traj(_ptr(a), _ptr(b), _ptr(v), n, levels, lo, hi, ADMM_TOL, 100 * levels,
                                             _ptr(state), _ptr(pred), _ptr(ws), ws.numel(), self.stream),
              "effq_fixed_point_traj")

    def fixed_point_bucket_rec(self, a, b, v, levels: int, state, pred, lo: float = -1.0, hi: float = 1.0):
        n = a.numel()
        ws = self._workspace("fp_bucket", self.lib.effq_fp_bucket_ws_bytes(n))
        check(self.lib.effq_fixed_point_bucket_rec(_ptr(a), _ptr(b), _ptr(v), n, levels, lo, hi, ADMM_TOL, 100 * levels,
                                                   _ptr(state), _ptr(ws), ws.numel(), _ptr(pred), self.stream),
              "effq_fixed_point_bucket_rec")

    def fixed_point_coop_rec(self, a, b, v, levels: int, state, pred, lo: float = -1.0, hi: float = 1.0):
        check(self.lib.effq_fixed_point_coop_rec(_ptr(a), _ptr(b), _ptr(v), a.numel(), levels, lo, hi, ADMM_TOL,
                                                 100 * levels, _ptr(state), _ptr(self._red_ws), _ptr(pred), self.stream),
              "effq_fixed_point_coop_rec")

    @staticmethod
    def read_fp_pred(pred: torch.Tensor):
        """FptPred of csrc/fp_level.h as a dict (tests, diagnostics)."""
        i32 = pred[:16].view(torch.int32).cpu()
        f = pred[16:16 + 8 * 40].view(torch.float64).cpu()
        i64 = pred[16 + 8 * 40:16 + 8 * 45].view(torch.int64).cpu()
        fn = pred[16 + 8 * 45:16 + 8 * 53].view(torch.float64).cpu()
        j64 = pred[16 + 8 * 53:16 + 8 * 63].view(torch.int64).cpu()
        K = int(i32[0])
        return {"K": K, "e": int(i32[1]), "e_valid": int(i32[2]), "lo": f[0:8].tolist(), "hi": f[8:16].tolist(),
                "eps": f[16:24].tolist(),
                "eps_n": fn.tolist(), "calls": int(i64[0]), "warm_iters": int(i64[1]), "full_iters": int(i64[2]),
                "listed": int(i64[3]), "list_max": int(i64[4]), "ring_iters": int(j64[0]), "ring_listed": int(j64[1]),
                "trace_us": [(int(j64[2 + k]) - int(j64[2])) / 100.0 for k in range(5)],
                "mean_us_phase1_setup_loop": [int(j64[7 + k]) / 100.0 / max(int(i64[0]), 1) for k in range(3)]}

    def fp_check(self, state, err_flag):
        check(self.lib.effq_fp_check(_ptr(state), _ptr(err_flag), self.stream), "effq_fp_check")

    # -- a5/a6 --------------------------------------------------------------------------------
    def gram(self, x_ndhwc: torch.Tensor, att: Optional[torch.Tensor], y_ndhwc: torch.Tensor, geom: Geom,
             has_bias: bool, A0: Optional[torch.Tensor] = None, B0: Optional[torch.Tensor] = None):
        """A0 (n x n), B0 (c2 x n) of solver.py:282-314, reference row order.  Accumulates when A0/B0 given."""
        x = self._f32(x_ndhwc)
        y = self._f32(y_ndhwc)
        a = self._f32(att) if att is not None else None
        _check_shapes(geom, x, y=y, att=a)
        n = geom.C1 * geom.KD * geom.KH * geom.KW + int(has_bias)
        acc = int(A0 is not None)
        if A0 is not None and (tuple(A0.shape) != (n, n) or tuple(B0.shape) != (geom.C2, n)):
            raise _lib.EffqError("gram: A0/B0 shapes do not match the geometry")
        if A0 is None:
            A0 = torch.empty(n, n, dtype=torch.float32, device=self.device)
            B0 = torch.empty(geom.C2, n, dtype=torch.float32, device=self.device)
        need = self.lib.effq_gram_ws_bytes(C.byref(geom), int(has_bias))
        ws = self._workspace("gram", need)
        check(self.lib.effq_gram_accum(_ptr(x), _ptr(a), _ptr(y), C.byref(geom), int(has_bias), _ptr(A0), _ptr(B0),
                                       acc, _ptr(ws), ws.numel(), self.stream), "effq_gram_accum")
        return A0, B0

    def gram_plan(self, geom: Geom, has_bias: bool) -> dict:
        """The launch gram() makes for a geometry (effq_gram_plan_query; launches nothing)."""
        vec, nb, npairs, nsplit, fold, fin = (C.c_int() for _ in range(6))
        vps = C.c_longlong()
        check(self.lib.effq_gram_plan_query(C.byref(geom), int(has_bias), C.byref(vec), C.byref(nb), C.byref(npairs),
                                            C.byref(nsplit), C.byref(vps), C.byref(fold), C.byref(fin)),
              "effq_gram_plan_query")
        return dict(vec=bool(vec.value), NB=nb.value, npairs=npairs.value, nsplit=nsplit.value, vox_per_split=vps.value,
                    fold=fold.value, finish_blocks=fin.value)

    def gram_streamed(self, x_ndhwc: torch.Tensor, y_ndhwc: torch.Tensor, geom: Geom, has_bias: bool) -> bool:
        """Whether gram() gathers these inputs with its streamed kernel (effq_gram_streamed; launches nothing)."""
        return bool(self.lib.effq_gram_streamed(_ptr(x_ndhwc), _ptr(y_ndhwc), C.byref(geom), int(has_bias)))

    def gram_i8_plan(self, geom: Geom, ncls: int = 1, n_list: int = 0) -> dict:
        """The launch gram_i8() makes for a geometry, ncls classes and a voxel list of n_list slots (0: no list)
        (effq_gram_i8_plan_query; launches nothing)."""
        out = [C.c_int() for _ in range(6)]
        check(self.lib.effq_gram_i8_plan_query(C.byref(geom), int(ncls), int(n_list), *[C.byref(o) for o in out]),
              "effq_gram_i8_plan_query")
        return dict(zip(("NB", "NBX", "npairs", "nchunks", "cps", "nsplit"), (o.value for o in out)))

    def gram_i8_groups(self, geom: Geom, ncls: int = 1, n_list: int = 0) -> dict:
        """Which block pairs of gram_i8_plan() one workgroup of gram_i8() computes: gi x gj adjacent blocks, ngroups x
        grid_y workgroups (effq_gram_i8_group_query; launches nothing)."""
        out = [C.c_int() for _ in range(4)]
        check(self.lib.effq_gram_i8_group_query(C.byref(geom), int(ncls), int(n_list), *[C.byref(o) for o in out]),
              "effq_gram_i8_group_query")
        return dict(zip(("gi", "gj", "ngroups", "grid_y"), (o.value for o in out)))

    def gram_i8_set_group(self, gi: int, gj: int) -> None:
        """Process-wide override of the grouping rule (test hook): (1, 1) one pair per workgroup, (0, 0) the rule."""
        check(self.lib.effq_gram_i8_set_group(int(gi), int(gj)), "effq_gram_i8_set_group")

    def gram_f64_plan(self, geom: Geom, has_bias: bool) -> dict:
        """The launch gram_f64() makes for a supported geometry (effq_gram_f64_plan_query; launches nothing)."""
        out = [C.c_int() for _ in range(4)]
        check(self.lib.effq_gram_f64_plan_query(C.byref(geom), int(has_bias), *[C.byref(o) for o in out]),
              "effq_gram_f64_plan_query")
        return dict(zip(("nchunk", "grid", "ntiles", "tpw"), (o.value for o in out)))

    def gram_i8_supported(self, geom: Geom, act_levels: int) -> bool:
        return bool(self.lib.effq_gram_i8_supported(C.byref(geom), int(act_levels)))

    GRAM_I8_MAX_CLASSES = 16

    def att_classes(self, att: Optional[torch.Tensor]):
        """Voxel list sorted by attention weight for effq_gram_accum_i8: (vox_list int32 padded per class to
        multiples of 128 with -1, chunk_cls int32, cls_w float32, ncls).  None when the mask has more distinct
        values than the kernel takes (the caller then uses the fp32 Gram).  Built by the library (effq_att_classes);
        cached per mask tensor, the pyramid level is shared by several layers."""
        if att is None:
            return (None, None, None, 1)
        key = (att.data_ptr(), att.numel(), att._version)
        hit = self._att_cache.get(key)
        if hit is not None:
            return hit[1]
        flat = self._f32(att).reshape(-1)
        V = flat.numel()
        lst = torch.empty(V + 128 * self.GRAM_I8_MAX_CLASSES, dtype=torch.int32, device=flat.device)
        chunk_cls = torch.empty(V // 128 + self.GRAM_I8_MAX_CLASSES, dtype=torch.int32, device=flat.device)
        cls_w = torch.empty(self.GRAM_I8_MAX_CLASSES, dtype=torch.float32, device=flat.device)
        info = (C.c_int32 * 3)()
        ws = self._workspace("att_cls", self.lib.effq_att_classes_ws_bytes())
        check(self.lib.effq_att_classes(_ptr(flat), V, _ptr(lst), _ptr(chunk_cls), _ptr(cls_w), info, _ptr(ws),
                                        self.stream), "effq_att_classes")
        k, n_list, overflow = int(info[0]), int(info[1]), int(info[2])
        res = None if overflow else (lst[:n_list], chunk_cls[: n_list // 128], cls_w[:k], k)
        if len(self._att_cache) > 16:
            self._att_cache.clear()
        self._att_cache[key] = (att, res)     # holding the mask keeps its address from being reused
        return res

    def gram_i8(self, xidx_ndhwc: torch.Tensor, att_cls, y_ndhwc: torch.Tensor, geom: Geom, has_bias: bool,
                act_alpha: torch.Tensor, act_levels: int, A0: Optional[torch.Tensor] = None,
                B0: Optional[torch.Tensor] = None, unweighted: bool = False):
        """A0/B0 of gram() for an already quantised input, exact on the i8 matrix cores (effq_gram_accum_i8).
        att_cls = att_classes(att).  unweighted=True also returns (Au, Bu): the same sums without the attention weights,
        fp64, no factor 2 - the operands of gram_loss()."""
        if xidx_ndhwc.dtype != torch.uint8 or not xidx_ndhwc.is_contiguous():
            raise _lib.EffqError("gram_i8 wants contiguous uint8 level ids")
        y = self._f32(y_ndhwc)
        _check_shapes(geom, xidx_ndhwc, y=y)
        lst, chunk_cls, cls_w, ncls = att_cls
        if lst is not None:
            od, oh, ow = geom.out_dims()
            if (int(lst.numel()) < geom.N * od * oh * ow or lst.numel() % 128 or
                    chunk_cls.numel() * 128 != lst.numel() or cls_w.numel() != ncls):
                raise _lib.EffqError("gram_i8: voxel list does not match the output volume")
        n = geom.C1 * geom.KD * geom.KH * geom.KW + int(has_bias)
        acc = int(A0 is not None)
        if A0 is not None and (tuple(A0.shape) != (n, n) or tuple(B0.shape) != (geom.C2, n)):
            raise _lib.EffqError("gram_i8: A0/B0 shapes do not match the geometry")
        if A0 is None:
            A0 = torch.empty(n, n, dtype=torch.float32, device=self.device)
            B0 = torch.empty(geom.C2, n, dtype=torch.float32, device=self.device)
        al = self._f32(act_alpha.reshape(1))
        ws = self._workspace("gram_i8", self.lib.effq_gram_i8_ws_bytes(C.byref(geom), int(ncls)))
        Au = Bu = None
        if unweighted:
            if acc:
                raise _lib.EffqError("gram_i8: the unweighted system is not accumulated across calls here")
            Au = torch.empty(n, n, dtype=torch.float64, device=self.device)
            Bu = torch.empty(geom.C2, n, dtype=torch.float64, device=self.device)
        check(self.lib.effq_gram_accum_i8_unw(_ptr(xidx_ndhwc), _ptr(y), C.byref(geom), int(has_bias), _ptr(al),
                                              int(act_levels), _ptr(lst), _ptr(chunk_cls), _ptr(cls_w), int(ncls),
                                              0 if lst is None else int(lst.numel()), _ptr(A0), _ptr(B0), acc,
                                              _ptr(Au), _ptr(Bu), _ptr(ws), ws.numel(), self.stream),
              "effq_gram_accum_i8_unw")
        return (A0, B0, Au, Bu) if unweighted else (A0, B0)

    def gram_f64_supported(self, geom: Geom, has_bias: bool) -> bool:
        return bool(self.lib.effq_gram_f64_supported(C.byref(geom), int(has_bias)))

    def gram_f64_pipelined(self, x_ndhwc: torch.Tensor, y_ndhwc: torch.Tensor, geom: Geom, has_bias: bool) -> bool:
        """Whether gram_f64() gathers these inputs with its pipelined loop (effq_gram_f64_pipelined; launches nothing)."""
        return bool(self.lib.effq_gram_f64_pipelined(_ptr(x_ndhwc), _ptr(y_ndhwc), C.byref(geom), int(has_bias)))

    def gram_f64(self, x_ndhwc: torch.Tensor, y_ndhwc: torch.Tensor, geom: Geom, has_bias: bool):
        """(Au, Bu): the unweighted fp64 Gram system of a layer with full-precision input (effq_gram_f64) - the
        operands of gram_loss() for the first conv and the classifier."""
        x, y = self._f32(x_ndhwc), self._f32(y_ndhwc)
        _check_shapes(geom, x, y=y)
        n = geom.C1 * geom.KD * geom.KH * geom.KW + int(has_bias)
        Au = torch.empty(n, n, dtype=torch.float64, device=self.device)
        Bu = torch.empty(geom.C2, n, dtype=torch.float64, device=self.device)
        ws = self._workspace("gram_f64", self.lib.effq_gram_f64_ws_bytes(C.byref(geom), int(has_bias)))
        check(self.lib.effq_gram_f64(_ptr(x), _ptr(y), C.byref(geom), int(has_bias), _ptr(Au), _ptr(Bu), _ptr(ws),
                                     ws.numel(), self.stream), "effq_gram_f64")
        return Au, Bu

    def upsample_trilinear(self, x_ndhwc: torch.Tensor, scale) -> torch.Tensor:
        """nn.Upsample(scale_factor=scale, mode='trilinear') on an NDHWC tensor (effq_upsample_trilinear)."""
        x = self._f32(x_ndhwc)
        N, D, H, W, Cc = (int(i) for i in x.shape)
        sd, sh, sw = (int(i) for i in scale)
        out = torch.empty(N, D * sd, H * sh, W * sw, Cc, dtype=torch.float32, device=self.device)
        check(self.lib.effq_upsample_trilinear(_ptr(x), N, D, H, W, Cc, sd, sh, sw, _ptr(out), self.stream),
              "effq_upsample_trilinear")
        return out

    def gram_loss(self, Au: torch.Tensor, Bu: torch.Tensor, syy: torch.Tensor, G: torch.Tensor, b, sqerr=None):
        """Squared error of conv(Qx, G, b) against the FP target from the unweighted Gram system (effq_gram_loss)."""
        c2, n = (int(i) for i in Bu.shape)
        has_b = b is not None
        if (Au.dtype != torch.float64 or Bu.dtype != torch.float64 or syy.dtype != torch.float64 or
                tuple(Au.shape) != (n, n) or G.numel() != c2 * (n - int(has_b))):
            raise _lib.EffqError("gram_loss: operand shapes / dtypes do not match")
        if sqerr is None:
            sqerr = torch.zeros(2, dtype=torch.float64, device=self.device)
        ws = self._workspace("gram_loss", self.lib.effq_gram_loss_ws_bytes(n))
        check(self.lib.effq_gram_loss(_ptr(Au), _ptr(Bu), _ptr(syy), _ptr(self._f32(G)), _ptr(b), c2, n, int(has_b),
                                      _ptr(sqerr), _ptr(ws), ws.numel(), self.stream), "effq_gram_loss")
        return sqerr

    def gram_loss_i8_supported(self, c2: int, n: int, has_b: bool, w_levels: int) -> bool:
        return bool(self.lib.effq_gram_loss_i8_supported(int(c2), int(n), int(has_b), int(w_levels)))

    def gram_loss_i8_planes(self, Au: torch.Tensor, has_b: bool, act_alpha: torch.Tensor, act_levels: int, voxels: int):
        """Balanced base-256 digit planes of K = Aww / s_a^2 (effq_gram_loss_i8_prepare): [P][round_up(nw, 256)][nw] int8.
        `voxels` bounds the entries: K <= (act_levels - 1)^2 * voxels.  Returns None if they need more than 6 planes."""
        n = int(Au.shape[0])
        P = self.lib.effq_gram_loss_i8_num_planes(int((act_levels - 1) ** 2 * voxels))
        if P < 1:
            return None
        nw = n - int(has_b)
        planes = torch.empty(P, (nw + 255) // 256 * 256, nw, dtype=torch.int8, device=self.device)
        assert planes.numel() == self.lib.effq_gram_loss_i8_planes_bytes(n, int(has_b), P)
        err = torch.zeros(1, dtype=torch.int32, device=self.device)
        al = self._f32(act_alpha.reshape(1))
        check(self.lib.effq_gram_loss_i8_prepare(_ptr(Au), n, int(has_b), _ptr(al), int(act_levels), P, _ptr(planes),
                                                 _ptr(err), self.stream), "effq_gram_loss_i8_prepare")
        planes._effq_err = err           # read with the layer's one host read (admm_read) or by the caller
        return planes

    def gram_loss_i8(self, planes, Au, Bu, syy, Gq, b, states, act_alpha, act_levels: int, w_levels: int, hist=None):
        """Losses of `count` stacked iterates (Gq [count, c2, nw] int8, b [count, c2], states [count, 5] fp64)."""
        count, c2 = int(Gq.shape[0]), int(Bu.shape[0])
        n = int(Bu.shape[1])
        has_b = b is not None
        if hist is None:
            hist = torch.zeros(count, 2, dtype=torch.float64, device=self.device)
        ws = self._workspace("gram_loss_i8", self.lib.effq_gram_loss_i8_ws_bytes())
        al = self._f32(act_alpha.reshape(1))
        check(self.lib.effq_gram_loss_i8(_ptr(planes), int(planes.shape[0]), _ptr(Au), _ptr(Bu), _ptr(syy), _ptr(Gq), _ptr(b),
                                         _ptr(states), _ptr(al), int(act_levels), int(w_levels), c2, n, int(has_b), count,
                                         _ptr(hist), _ptr(ws), ws.numel(), self.stream), "effq_gram_loss_i8")
        return hist

    def gram_reduce(self, A0: torch.Tensor, B0: torch.Tensor, reducer):
        """Data-parallel SUM of a layer's Gram system as ONE message: upper triangle of A0 + B0 (effq_gram_pack)."""
        n, c2 = int(A0.shape[0]), int(B0.shape[0])
        buf = torch.empty(self.lib.effq_gram_packed_elems(n, c2), dtype=torch.float32, device=self.device)
        check(self.lib.effq_gram_pack(_ptr(A0), _ptr(B0), n, c2, _ptr(buf), self.stream), "effq_gram_pack")
        reducer(buf)
        check(self.lib.effq_gram_unpack(_ptr(buf), n, c2, _ptr(A0), _ptr(B0), self.stream), "effq_gram_unpack")
        return A0, B0

    # -- f2: bit-packed level ids -------------------------------------------------------------
    @staticmethod
    def storage_bits(levels: int) -> int:
        """Smallest supported field width (1/2/4/8 bits) that holds `levels` level ids."""
        for b in (1, 2, 4, 8):
            if levels <= (1 << b):
                return b
        raise _lib.EffqError(f"{levels} levels do not fit 8 bits")

    def pack_levels(self, idx: torch.Tensor, bits: int) -> torch.Tensor:
        if idx.dtype != torch.uint8 or not idx.is_contiguous():
            raise _lib.EffqError("pack_levels wants contiguous uint8 level ids")
        nb = self.lib.effq_packed_bytes(idx.numel(), int(bits))
        if idx.numel() and nb == 0:
            raise _lib.EffqError(f"unsupported field width {bits}")
        out = torch.empty(int(nb), dtype=torch.uint8, device=idx.device)
        check(self.lib.effq_pack_levels(_ptr(idx), idx.numel(), int(bits), _ptr(out), self.stream), "effq_pack_levels")
        return out

    def unpack_levels(self, packed: torch.Tensor, n: int, bits: int) -> torch.Tensor:
        if packed.dtype != torch.uint8 or packed.numel() != self.lib.effq_packed_bytes(int(n), int(bits)):
            raise _lib.EffqError("unpack_levels: buffer does not match n and the field width")
        out = torch.empty(int(n), dtype=torch.uint8, device=packed.device)
        check(self.lib.effq_unpack_levels(_ptr(packed.contiguous()), int(n), int(bits), _ptr(out), self.stream),
              "effq_unpack_levels")
        return out

    # -- a7 -----------------------------------------------------------------------------------
    def spd_inverse(self, A0: torch.Tensor, has_bias: bool, rho: float, eta: float,
                    out: Optional[torch.Tensor] = None, ws_key: str = "inv") -> torch.Tensor:
        n = A0.shape[0]
        A0 = self._f32(A0)
        if out is None:     # n rows of effq_ainv_ld(n) floats (zero padded, 16-byte aligned rows)
            out = torch.empty(n, self.lib.effq_ainv_ld(n), dtype=torch.float32, device=self.device)
        ws = self._workspace(ws_key, self.lib.effq_spd_inverse_ws_bytes(n))
        check(self.lib.effq_spd_inverse(_ptr(A0), n, int(has_bias), rho, eta, _ptr(out), _ptr(ws), ws.numel(),
                                        self.stream), "effq_spd_inverse")
        return out

    def spd_inverse_plan(self, n: int) -> dict:
        """The sweep spd_inverse takes for n rows (effq_spd_inverse_plan; launches nothing)."""
        wide, nblk, piv = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.effq_spd_inverse_plan(int(n), C.byref(wide), C.byref(nblk), C.byref(piv)), "effq_spd_inverse_plan")
        return dict(wide=bool(wide.value), nblk=nblk.value, pivot_blocks=piv.value)

    def prox_plan(self, c2: int, n: int) -> dict:
        """The GEMM variant, grid and K split prox_solve takes for a c2 x n system (effq_prox_plan_query; launches nothing)."""
        v, gx, gy, ns = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self.lib.effq_prox_plan_query(int(c2), int(n), C.byref(v), C.byref(gx), C.byref(gy), C.byref(ns)),
              "effq_prox_plan_query")
        return dict(variant=v.value, gx=gx.value, gy=gy.value, nsplit=ns.value)

    def prox_solve(self, B0, Ainv, W0, b0, G, dual, rho: float, eta: float, wstar, bstar):
        c2, n = B0.shape
        ws = self._workspace("prox", self.lib.effq_prox_ws_bytes(c2, n))
        check(self.lib.effq_prox_solve(_ptr(B0), _ptr(Ainv), _ptr(W0), _ptr(b0), _ptr(G), _ptr(dual), c2, n,
                                       int(b0 is not None), rho, eta, _ptr(wstar), _ptr(bstar), _ptr(ws),
                                       ws.numel(), self.stream), "effq_prox_solve")

    PROX_SHIFT_TERMS = 26      # contraction factor < 1/2 per sweep: 2^-26 is below fp32 resolution

    def prox_solve_shifted(self, B0, Ainv, W0, b0, G, dual, rho: float, eta: float, rho_inv: float, wstar, bstar):
        """prox_solve for A(rho) through the inverse of A(rho_inv), rho_inv >= rho (effq_prox_solve_shifted)."""
        c2, n = B0.shape
        ws = self._workspace("prox", self.lib.effq_prox_ws_bytes(c2, n))
        # sweeps for 2^-26: factor <= d/(rho_inv+eta)
        terms = self.shift_terms(rho, eta, rho_inv)
        check(self.lib.effq_prox_solve_shifted(_ptr(B0), _ptr(Ainv), _ptr(W0), _ptr(b0), _ptr(G), _ptr(dual), c2, n,
                                               int(b0 is not None), rho, eta, rho_inv, terms, _ptr(wstar),
                                               _ptr(bstar), _ptr(ws), ws.numel(), self.stream),
              "effq_prox_solve_shifted")

    # -- the whole ADMM loop of a layer in one binding call ---------------------------------------------
    def admm_run(self, A0, B0, W0, b0, geom: Geom, y_ndhwc, *, xq=None, xidx=None, act_alpha=None, act_levels: int = 0,
                 loss_kind: int = 0, rho: float, rho_max: float, eta: float, iters: int, period: int, levels: int,
                 overlap: bool = True, loss_gram=None, residuals: bool = False, channel_wise: bool = False):
        """effq_admm_run: enqueue `iters` ADMM iterations (chain on the current stream, per-iteration loss on the
        loss stream, later inverses on the side stream).  Returns a handle with the rings and `hist` (iters x 2
        device doubles, sums of squared errors); no host synchronisation.
        Memory: every iterate is kept until the best one is picked after the loop (G_ring: iters x nw floats, plus an
        int8 copy where the loss is an integer conv): 1.75 GB for a 256 -> 256 3^3 layer, 7 GB for LiTS' 512 -> 512,
        linear in `iters` (200 in the reference, a constructor constant there) - of 288 GB; the reference keeps one
        best iterate but synchronises with the host every iteration to do so.
        channel_wise: one weight scale per output channel (effq_fixed_point_channels_proj); the run then carries
        `alpha_ring` (iters x c2 doubles) and `w_iters_ring` (iters x c2 int32).  Loss kinds 0 and 4 only."""
        from types import SimpleNamespace
        c2, n = (int(i) for i in B0.shape)
        has_b = b0 is not None
        # convert ONCE and keep the converted tensors alive with the run (the call only enqueues work on three streams:
        # a temporary .contiguous() copy could be handed back to the allocator while kernels still read it)
        W0, A0, B0 = self._f32(W0), self._f32(A0), self._f32(B0)
        b0 = self._f32(b0) if has_b else None
        xq = self._f32(xq) if xq is not None else None
        nw = W0.numel()
        y = self._f32(y_ndhwc)
        planes = None
        if loss_gram is not None and len(loss_gram) == 4:
            loss_kind = 5                         # (Au, Bu, syy, planes): the same with the quadratic form on the i8 cores
            planes = loss_gram[3]
            loss_gram = loss_gram[:3]
        elif loss_gram is not None:
            loss_kind = 4                         # (Au, Bu, syy): losses from the unweighted Gram system
        if channel_wise and loss_kind not in (0, 4):
            raise _lib.EffqError(f"admm_run: channel mode takes loss kinds 0 and 4, not {loss_kind}")
        _check_shapes(geom, xq if loss_kind in (0, 4, 5) else xidx, W0, b0, y)
        if tuple(A0.shape) != (n, n) or nw != c2 * (n - int(has_b)):
            raise _lib.EffqError("admm_run: A0/B0/W0 shapes do not match")
        n_inv = self.lib.effq_admm_num_inverses(float(rho), float(rho_max), int(iters), int(period))
        if n_inv < 1:
            raise _lib.EffqError("admm_run: bad rho schedule")
        dev, f32 = self.device, torch.float32
        ld = self.lib.effq_ainv_ld(n)
        r = SimpleNamespace(iters=int(iters), nw=nw, c2=c2, has_b=has_b, channel_wise=bool(channel_wise))
        r.ainv = torch.empty(n_inv, n, ld, dtype=f32, device=dev)
        r.dual = torch.empty(nw, dtype=f32, device=dev)
        r.wstar = torch.empty(nw, dtype=f32, device=dev)
        r.v = torch.empty(nw, dtype=f32, device=dev)
        r.G_ring = torch.empty(iters, nw, dtype=f32, device=dev)
        r.Gq_ring = torch.empty(iters, nw, dtype=torch.int8, device=dev) if loss_kind in (1, 2, 5) else None
        r.b_ring = torch.empty(iters, c2, dtype=f32, device=dev) if has_b else None
        r.state_ring = torch.zeros(iters, 5, dtype=torch.float64, device=dev)
        r.hist = torch.zeros(iters, 2, dtype=torch.float64, device=dev)
        r.err = torch.zeros(1, dtype=torch.int32, device=dev)
        r.res = torch.zeros(iters, 2, dtype=torch.float64, device=dev) if residuals else None     # lwq_verbose
        r.alpha_ring = torch.zeros(iters, c2, dtype=torch.float64, device=dev) if channel_wise else None
        r.w_iters_ring = torch.zeros(iters, c2, dtype=torch.int32, device=dev) if channel_wise else None
        main = torch.cuda.current_stream(dev)
        loss_s = self.loss_stream() if overlap else None
        side_s = self.side_stream()
        # workspaces are (zero-)filled on the current stream, ahead of the events the library orders the other
        # streams by
        prox = self._workspace("prox", self.lib.effq_prox_ws_bytes(c2, n))
        inv = self._workspace("inv", self.lib.effq_spd_inverse_ws_bytes(n))
        inv_side = (self._workspace("inv_side", self.lib.effq_spd_inverse_ws_bytes(n))
                    if n_inv > 1 else None)
        inv_side2 = (self._workspace("inv_side2", self.lib.effq_spd_inverse_ws_bytes(n))
                     if n_inv > 2 else None)
        fpw = (self._workspace("fp_bucket", self.lib.effq_fp_bucket_ws_bytes(nw))
               if nw <= self.lib.effq_fp_bucket_max() and not channel_wise else None)
        # weight projection from the previous iteration's iterates (effq_fixed_point_traj)
        traj = not channel_wise and bool(self.lib.effq_admm_uses_traj(nw, int(levels)))   # the library's own decision
        tws = self._workspace("fp_traj", self.lib.effq_fp_traj_ws_bytes(nw)) if traj else None
        r.fp_pred = torch.zeros(self.lib.effq_fp_traj_pred_bytes(), dtype=torch.uint8, device=dev) if traj else None
        if loss_kind == 5:
            cws = self._workspace("gram_loss_i8", self.lib.effq_gram_loss_i8_ws_bytes())
        elif loss_kind == 4:
            cws = self._workspace("gram_loss", self.lib.effq_gram_loss_ws_bytes(n))
        elif loss_kind == 1:
            cws = self._workspace("conv_i8", self.lib.effq_conv_i8_ws_bytes(C.byref(geom)))
        elif loss_kind == 2:
            cws = self._workspace("conv_i8s", self.lib.effq_conv_i8s_ws_bytes(C.byref(geom), int(act_levels),
                                                                             int(levels)))
        else:
            cws = self._workspace("conv", self.lib.effq_conv_ws_bytes(C.byref(geom)))
        al = self._f32(act_alpha.reshape(1)) if (act_alpha is not None and loss_kind in (1, 2, 5)) else None
        a = _lib.AdmmRunArgs()
        p = lambda t: None if t is None else t.data_ptr()
        a.A0, a.B0, a.W0, a.b0 = p(A0), p(B0), p(W0), p(b0)
        a.c2, a.n, a.has_bias, a.w_levels = c2, n, int(has_b), int(levels)
        a.iters, a.rho_period = int(iters), int(period)
        a.rho, a.rho_max, a.eta, a.tol = float(rho), float(rho_max), float(eta), ADMM_TOL
        a.geom = geom
        a.loss_kind, a.act_levels = int(loss_kind), int(act_levels)
        a.xq = p(xq) if loss_kind == 0 else None
        a.xidx = p(xidx) if loss_kind in (1, 2) else None
        if loss_kind in (4, 5):
            Au, Bu, syy = loss_gram
            if (Au.dtype != torch.float64 or Bu.dtype != torch.float64 or syy.dtype != torch.float64 or
                    tuple(Au.shape) != (n, n) or tuple(Bu.shape) != (c2, n) or syy.numel() != 1):
                raise _lib.EffqError("admm_run: loss_gram wants fp64 (Au [n,n], Bu [c2,n], syy [1])")
            a.loss_Au, a.loss_Bu, a.loss_syy = p(Au), p(Bu), p(syy)
            if loss_kind == 5:
                a.loss_planes, a.loss_nplanes = p(planes), int(planes.shape[0])
                r.loss_planes = planes
        a.y_fp, a.act_alpha_dev = p(y), p(al)
        a.dual, a.wstar, a.v = p(r.dual), p(r.wstar), p(r.v)
        a.G_ring, a.Gq_ring, a.b_ring = p(r.G_ring), p(r.Gq_ring), p(r.b_ring)
        a.state_ring, a.hist, a.err_flag = p(r.state_ring), p(r.hist), p(r.err)
        a.res_ring = p(r.res)
        a.channel_wise, a.alpha_ring, a.w_iters_ring = int(bool(channel_wise)), p(r.alpha_ring), p(r.w_iters_ring)
        a.ainv_pool, a.n_ainv = p(r.ainv), n_inv
        a.prox_ws, a.prox_ws_bytes = p(prox), prox.numel()
        a.red_ws = p(self._red_ws)
        a.fp_ws, a.fp_ws_bytes = p(fpw), (fpw.numel() if fpw is not None else 0)
        a.fp_pred, a.fp_traj_ws, a.fp_traj_ws_bytes = p(r.fp_pred), p(tws), (tws.numel() if tws is not None else 0)
        a.inv_ws, a.inv_ws_bytes = p(inv), inv.numel()
        a.inv_ws_side, a.inv_ws_side_bytes = p(inv_side), (inv_side.numel() if inv_side is not None else 0)
        a.conv_ws, a.conv_ws_bytes = p(cws), cws.numel()
        a.stream_main = main.cuda_stream
        a.stream_loss = loss_s.cuda_stream if loss_s is not None else None
        a.stream_side = side_s.cuda_stream if inv_side is not None else None
        if inv_side2 is not None:
            a.stream_side2 = self.side_stream2().cuda_stream
            a.inv_ws_side2, a.inv_ws_side2_bytes = p(inv_side2), inv_side2.numel()
        r.keep = (A0, B0, W0, b0, y, xq, xidx, al, loss_gram)       # the call only enqueues: keep every operand alive
        check(self.lib.effq_admm_run(C.byref(a)), "effq_admm_run")
        return r

    def admm_select_best(self, run):
        """Earliest iterate with the smallest (already all-reduced) loss: (best_G, best_b, best[loss sum, index])."""
        best_G = torch.empty(run.nw, dtype=torch.float32, device=self.device)
        best_b = torch.empty(run.c2, dtype=torch.float32, device=self.device) if run.has_b else None
        best = torch.empty(2, dtype=torch.float64, device=self.device)
        check(self.lib.effq_admm_select_best(_ptr(run.hist), run.iters, _ptr(run.G_ring), _ptr(run.b_ring), run.nw,
                                             run.c2, _ptr(best_G), _ptr(best_b), _ptr(best), self.stream),
              "effq_admm_select_best")
        return best_G, best_b, best

    @staticmethod
    def admm_read(run, best, extra=None):
        """ONE device->host copy per layer: loss history, best, the last scale, fixed-point iteration counts, error
        (and `extra`, a small fp64 device tensor the caller wants read in the same copy)."""
        err = run.err.to(torch.float64)
        if getattr(run, "loss_planes", None) is not None:       # effq_gram_loss_i8_prepare's flag: 1000 x (1 | 2)
            err = err + 1000.0 * run.loss_planes._effq_err.to(torch.float64)
        if getattr(run, "channel_wise", False):
            return HipOps._admm_read_channels(run, best, err, extra)
        parts = [run.hist[:, 0], best, run.state_ring[-1, :1], run.state_ring[:, 4], err]
        if extra is not None:
            parts.append(extra.to(torch.float64).reshape(-1))
        pack = torch.cat(parts).cpu()
        it = run.iters
        w_iters = pack[it + 3: 2 * it + 3].contiguous().view(torch.int32)[0::2].tolist()
        return dict(hist=pack[:it].tolist(), best=pack[it:it + 2].tolist(), alpha_w=float(pack[it + 2]),
                    w_iters=w_iters, err=int(pack[2 * it + 3]),
                    extra=pack[2 * it + 4:].tolist() if extra is not None else None)

    @staticmethod
    def channel_alpha_best(run, best):
        """Channel mode: the BEST iterate's per-row scales (device-side index of the scale ring, no host read)."""
        return run.alpha_ring.index_select(0, best[1:2].to(torch.long)).reshape(-1)

    @staticmethod
    def _admm_read_channels(run, best, err, extra):
        """admm_read of a channel-mode run: alpha_w = the best iterate's scale vector, w_iters = the per-iteration maximum
        over the rows, w_iters_rows = the row that took it."""
        it, c2 = run.iters, run.c2
        wmax, wrow = run.w_iters_ring.max(dim=1)
        parts = [run.hist[:, 0], best, HipOps.channel_alpha_best(run, best), wmax.to(torch.float64),
                 wrow.to(torch.float64), err]
        if extra is not None:
            parts.append(extra.to(torch.float64).reshape(-1))
        pack = torch.cat(parts).cpu()
        o = it + 2
        a_w = pack[o:o + c2].tolist()
        o += c2
        w_iters = [int(v) for v in pack[o:o + it].tolist()]
        w_rows = [int(v) for v in pack[o + it:o + 2 * it].tolist()]
        o += 2 * it
        return dict(hist=pack[:it].tolist(), best=pack[it:it + 2].tolist(), alpha_w=a_w, w_iters=w_iters,
                    w_iters_rows=w_rows, err=int(pack[o]), extra=pack[o + 1:].tolist() if extra is not None else None)

    def fixed_point_channels(self, a, b, v, levels: int, alpha, iters=None, err_flag=None, proj=None):
        """effq_fixed_point_channels[_proj]: one scale per output row of a ([c2, ...]).  alpha: c2 device doubles; iters:
        c2 int32 (optional).  proj = dict(G, dual_div[, Bm, B0, W0, ldb, rho_next, eta]) runs the projection epilogue
        (then b is the dual, updated in place)."""
        c2 = int(a.shape[0])
        nwrow = a.numel() // c2
        tol, cap = ADMM_TOL, 100 * int(levels)
        if proj is None:
            check(self.lib.effq_fixed_point_channels(_ptr(a), _ptr(b), _ptr(v), c2, nwrow, int(levels), tol, cap,
                                                     _ptr(alpha), _ptr(iters), _ptr(err_flag), self.stream),
                  "effq_fixed_point_channels")
            return
        Bm = proj.get("Bm")
        B0 = proj.get("B0")
        check(self.lib.effq_fixed_point_channels_proj(
            _ptr(a), _ptr(b), _ptr(v), c2, nwrow, int(levels), tol, cap, _ptr(alpha), _ptr(iters), _ptr(err_flag),
            _ptr(proj["G"]), float(proj["dual_div"]), _ptr(Bm), _ptr(B0), _ptr(proj.get("W0")),
            int(B0.shape[1]) if B0 is not None else 0, int(proj.get("ldb", 0)), float(proj.get("rho_next", 0.0)),
            float(proj.get("eta", 0.0)), self.stream), "effq_fixed_point_channels_proj")

    def shift_terms(self, rho: float, eta: float, rho_inv: float) -> int:
        d = rho_inv - rho
        return 1 if d <= 0 else min(64, max(2, int(math.ceil(-26.0 * math.log(2.0) / math.log(d / (rho_inv + eta))))))

    # -- a4 elementwise -------------------------------------------------------------------------
    def admm_presum(self, wstar, dual, v):
        check(self.lib.effq_admm_presum(_ptr(wstar), _ptr(dual), _ptr(v), wstar.numel(), self.stream),
              "effq_admm_presum")

    def admm_project_dual(self, v, wstar, state, levels: int, G, dual, dual_div: float, Gq=None):
        check(self.lib.effq_admm_project_dual(_ptr(v), _ptr(wstar), _ptr(state), levels, _ptr(G), _ptr(dual),
                                              float(dual_div), _ptr(Gq), v.numel(), self.stream),
              "effq_admm_project_dual")

    def conv_plan(self, geom: Geom, loss_only: bool = False) -> dict:
        """The launch conv_step makes for a geometry (conv_plan_query)."""
        return conv_plan_query(self.lib, geom, loss_only)

    def conv_i8_plan(self, geom: Geom, want_out: bool = False) -> dict:
        """The launch conv_step_i8 (or, with want_out, conv_forward_i8) makes for a geometry (conv_i8_plan_query)."""
        return conv_i8_plan_query(self.lib, geom, want_out)

    def conv_i8s_plan(self, geom: Geom, act_levels: int, w_levels: int) -> dict:
        """The launch conv_step_i8s makes for a geometry and a level pair (conv_i8s_plan_query)."""
        return conv_i8s_plan_query(self.lib, geom, act_levels, w_levels)

    def conv_i8_supported(self, geom: Geom, act_levels: int, w_levels: int) -> bool:
        return bool(self.lib.effq_conv_i8_supported(C.byref(geom), int(act_levels), int(w_levels)))

    def conv_i8s_supported(self, geom: Geom, act_levels: int, w_levels: int) -> bool:
        return bool(self.lib.effq_conv_i8s_supported(C.byref(geom), int(act_levels), int(w_levels)))

    def conv_step_i8s(self, xidx: torch.Tensor, Gq: torch.Tensor, bias, geom: Geom, y_ndhwc: torch.Tensor,
                      act_alpha: torch.Tensor, act_levels: int, w_state: torch.Tensor, w_levels: int, sqerr,
                      prepare: bool):
        """Exact-integer loss evaluation for short-K layers and up to 256 levels (conv3d_calib_step_i8s).
        prepare=True on the first call of a layer (per-voxel level sums are cached in the workspace)."""
        if xidx.dtype != torch.uint8 or Gq.dtype != torch.int8:
            raise _lib.EffqError("conv_step_i8s wants uint8 level ids and int8 weight operands")
        _check_shapes(geom, xidx, Gq, bias, y_ndhwc)
        al = self._f32(act_alpha.reshape(1))
        ws = self._workspace("conv_i8s", self.lib.effq_conv_i8s_ws_bytes(C.byref(geom), int(act_levels), int(w_levels)))
        check(self.lib.conv3d_calib_step_i8s(_ptr(xidx), _ptr(Gq), _ptr(bias), _ptr(self._f32(y_ndhwc)),
                                             C.byref(geom), _ptr(al), int(act_levels), _ptr(w_state), int(w_levels),
                                             int(bool(prepare)), _ptr(sqerr), _ptr(ws), ws.numel(), self.stream),
              "conv3d_calib_step_i8s")
        return sqerr

    def conv_step_i8(self, xidx: torch.Tensor, Gq: torch.Tensor, bias, geom: Geom, y_ndhwc: torch.Tensor,
                     act_alpha: torch.Tensor, act_levels: int, w_state: torch.Tensor, w_levels: int, sqerr):
        """Exact-integer loss evaluation (conv3d_calib_step_i8)."""
        if xidx.dtype != torch.uint8 or Gq.dtype != torch.int8:
            raise _lib.EffqError("conv_step_i8 wants uint8 level ids and int8 weight numerators")
        _check_shapes(geom, xidx, Gq, bias, y_ndhwc)
        al = self._f32(act_alpha.reshape(1))
        ws = self._workspace("conv_i8", self.lib.effq_conv_i8_ws_bytes(C.byref(geom)))
        check(self.lib.conv3d_calib_step_i8(_ptr(xidx), _ptr(Gq), _ptr(bias), _ptr(self._f32(y_ndhwc)), C.byref(geom),
                                            _ptr(al), int(act_levels), _ptr(w_state), int(w_levels), _ptr(sqerr),
                                            _ptr(ws), ws.numel(), self.stream), "conv3d_calib_step_i8")
        return sqerr

    def conv_i8_out_supported(self, geom: Geom, act_levels: int, w_levels: int) -> bool:
        return bool(self.lib.effq_conv_i8_out_supported(C.byref(geom), int(act_levels), int(w_levels)))

    def conv_forward_i8(self, xidx: torch.Tensor, G: torch.Tensor, bias, geom: Geom, y_ndhwc: torch.Tensor, att,
                        act_alpha: torch.Tensor, act_levels: int, w_state: torch.Tensor, w_levels: int):
        """The quantised forward of a calibrated layer + its final loss on the i8 matrix cores (conv3d_quant_forward_i8):
        `G` = alpha_w * b, the projected weights of the iterate whose fixed-point state is `w_state` (5 device doubles,
        alpha first); returns (out NDHWC fp32, [sum err^2, sum att err^2] device doubles)."""
        if xidx.dtype != torch.uint8:
            raise _lib.EffqError("conv_forward_i8 wants uint8 level ids")
        att_f = self._f32(att) if att is not None else None
        _check_shapes(geom, xidx, G, bias, y_ndhwc, att_f)
        lm1 = int(w_levels) - 1
        a32 = w_state.reshape(-1)[0].to(torch.float32)
        # the integer numerators 2 * level - (Lw - 1) of the weights: G / f32(alpha) is b = level * d - 1 to an ulp
        Gq = (2.0 * torch.round((self._f32(G) / a32 + 1.0) * (0.5 * lm1)) - lm1).to(torch.int8).contiguous()
        al = self._f32(act_alpha.reshape(1))
        y = self._f32(y_ndhwc)
        out = torch.empty_like(y)
        sq = torch.zeros(2, dtype=torch.float64, device=self.device)
        st = w_state.to(torch.float64).contiguous()
        ws = self._workspace("conv_i8", self.lib.effq_conv_i8_ws_bytes(C.byref(geom)))
        check(self.lib.conv3d_quant_forward_i8(_ptr(xidx), _ptr(Gq), _ptr(self._f32(bias) if bias is not None else None),
                                               _ptr(y), _ptr(att_f), C.byref(geom), _ptr(al), int(act_levels), _ptr(st),
                                               int(w_levels), _ptr(sq), _ptr(out), _ptr(ws), ws.numel(), self.stream),
              "conv3d_quant_forward_i8")
        self._keep_i8 = (Gq, st, att_f, al)           # operands of an enqueued kernel: alive until the next call
        return out, sq

    # -- f3: gradients of the activation quantiser, Adam ----------------------------------------------------
    def act_quant_backward(self, x: torch.Tensor, alpha: torch.Tensor, levels: int, gq: torch.Tensor, want_gx=True):
        """(gx, galpha[device double]) of q = discretize(x/alpha, L, 0, 1)*alpha given gq (effq_act_quant_backward)."""
        x, gq = self._f32(x), self._f32(gq)
        a = self._f32(alpha.reshape(1))
        gx = torch.empty_like(x) if want_gx else None
        ga = torch.empty(1, dtype=torch.float64, device=self.device)
        check(self.lib.effq_act_quant_backward(_ptr(x), _ptr(a), int(levels), _ptr(gq), _ptr(gx), _ptr(ga), x.numel(),
                                               _ptr(self._red_ws), self.stream), "effq_act_quant_backward")
        return gx, ga

    def adam_step(self, p, g, m, v, lr: float, t: int, b1=0.9, b2=0.999, eps=1e-8):
        """torch.optim.Adam step in place on flat fp32 tensors (effq_adam_step); lr, betas and eps travel as doubles."""
        check(self.lib.effq_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), float(lr), float(b1), float(b2), float(eps),
                                      int(t), p.numel(),
                                      self.stream), "effq_adam_step")

    # -- the conv ---------------------------------------------------------------------------------
    def conv_step(self, x_ndhwc: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], geom: Geom,
                  y_ndhwc: Optional[torch.Tensor] = None, att: Optional[torch.Tensor] = None,
                  act_alpha: Optional[torch.Tensor] = None, act_levels: int = 0, want_out: bool = False,
                  sqerr: Optional[torch.Tensor] = None):
        """conv3d_quant_calib_step.  Returns (out NDHWC or None, sqerr device fp64[2] or None)."""
        x = self._f32(x_ndhwc)
        w = self._f32(weight)
        b = self._f32(bias) if bias is not None else None
        y = self._f32(y_ndhwc) if y_ndhwc is not None else None
        a = self._f32(att) if att is not None else None
        _check_shapes(geom, x, w, b, y, a)
        od, oh, ow = geom.out_dims()
        out = torch.empty(geom.N, od, oh, ow, geom.C2, dtype=torch.float32, device=self.device) if want_out else None
        if y is not None and sqerr is None:
            sqerr = torch.empty(2, dtype=torch.float64, device=self.device)
        al = self._f32(act_alpha.reshape(1)) if act_alpha is not None else None
        ws = self._workspace("conv", self.lib.effq_conv_ws_bytes(C.byref(geom)))
        check(self.lib.conv3d_quant_calib_step(_ptr(x), _ptr(w), _ptr(b), _ptr(y), _ptr(a), C.byref(geom), _ptr(al),
                                               int(act_levels), _ptr(sqerr), _ptr(out), _ptr(ws), ws.numel(),
                                               self.stream), "conv3d_quant_calib_step")
        return out, sqerr

    # -- validation on whole volumes (evaluate.validate_seg) ----------------------------------------------------
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
        if task == "lits":
            mode, lshape, thresh = _lib.SEG_ARGMAX, tuple(x.shape[1:]), 0.0
        elif task == "brats":
            mode, lshape, thresh = _lib.SEG_SIGMOID, tuple(x.shape), self.sigmoid_threshold()
        else:
            raise _lib.EffqError(f"Unknown task {task}")
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
        mode = {"lits": _lib.SEG_ARGMAX, "brats": _lib.SEG_SIGMOID}.get(task)
        if mode is None:
            raise _lib.EffqError(f"Unknown task {task}")
        grid, trips = C.c_int(0), C.c_int(0)
        check(self.lib.effq_seg_sweep_plan(int(Cc), int(S), mode, C.byref(grid), C.byref(trips)), "effq_seg_sweep_plan")
        return {"grid": grid.value, "trips": trips.value}

    def sweep_edges(self, kind: str) -> torch.Tensor:
        """The 4096 fp32 edges of seg_sweep's bins on the host (effq_seg_sweep_edges), index 0 = -inf: kind 'lits' /
        'argmax' (edge 2048 = 0) or 'brats' / 'sigmoid' (edge 2048 = the default sigmoid threshold)."""
        mode = {"argmax": _lib.SEG_ARGMAX, "lits": _lib.SEG_ARGMAX, "sigmoid": _lib.SEG_SIGMOID,
                "brats": _lib.SEG_SIGMOID}.get(kind)
        if mode is None:
            raise _lib.EffqError(f"sweep_edges: unknown kind {kind!r} (argmax or sigmoid)")
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
        if rule not in _lib.SEG_LABEL_RULES:
            raise _lib.EffqError(f"seg_labels: unknown rule {rule!r} (one of {', '.join(_lib.SEG_LABEL_RULES)})")
        fcode = self._fuse_code("seg_labels", fuse, rule == "argmax", f"rule {rule}", Cc, rule)
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
        if rule not in _lib.SEG_LABEL_RULES:
            raise _lib.EffqError(f"seg_labels_source: unknown rule {rule!r} (one of {', '.join(_lib.SEG_LABEL_RULES)})")
        fcode = self._fuse_code("seg_labels_source", fuse, rule == "argmax", f"rule {rule}", Cc, rule)
        try:
            lo, G, src = (tuple(int(v) for v in t) for t in (pmin, grid, source_shape))
            f = (1.0, 1.0, 1.0) if factors is None else tuple(float(v) for v in factors)
        except (TypeError, ValueError) as e:
            raise _lib.EffqError(f"seg_labels_source: {e}") from e
        if len(lo) != 3 or len(G) != 3 or len(src) != 3 or len(f) != 3 or x.numel() == 0:
            raise _lib.EffqError(f"seg_labels_source: box at {lo} of {tuple(x.shape[1:])}, grid {G}, factors {f}, source "
                                 f"{src}: three values each")
        if min(src) < 1 or max(src) > 32767 or math.prod(src) >= 2 ** 31:     # the output is not allocated for these
            raise _lib.EffqError(f"seg_labels_source: source grid {src}: 1 to 32767 along an axis, 2^31 - 1 voxels at most")
        out = torch.empty(src, dtype=torch.uint8, device=self.device)
        thresh = 0.0 if rule == "argmax" else self.sigmoid_threshold()
        i3 = C.c_int * 3
        check(self.lib.effq_seg_labels_source(_ptr(x), Cc, i3(*(int(v) for v in x.shape[1:])), i3(*lo), i3(*G),
                                              (C.c_double * 3)(*f), i3(*src), _lib.SEG_LABEL_RULES[rule],
                                              fcode, thresh, _ptr(out), self.stream), "effq_seg_labels_source")
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
        code = {"argmax": _lib.SEG_ARGMAX, "sigmoid": _lib.SEG_SIGMOID}.get(mode)
        if code is None:
            raise _lib.EffqError(f"seg_probs_source: unknown mode {mode!r} (argmax or sigmoid)")
        if not 0 < Cc <= _lib.SEG_TALLIES_MAX_CLASSES:
            raise _lib.EffqError(f"seg_probs_source: {Cc} classes, at most {_lib.SEG_TALLIES_MAX_CLASSES}")
        if not (want_prob or want_unc):
            raise _lib.EffqError("seg_probs_source: neither the probabilities nor the uncertainty is wanted")
        try:
            lo, G, src = (tuple(int(v) for v in t) for t in (pmin, grid, source_shape))
            f = (1.0, 1.0, 1.0) if factors is None else tuple(float(v) for v in factors)
        except (TypeError, ValueError) as e:
            raise _lib.EffqError(f"seg_probs_source: {e}") from e
        if len(lo) != 3 or len(G) != 3 or len(src) != 3 or len(f) != 3 or x.numel() == 0:
            raise _lib.EffqError(f"seg_probs_source: box at {lo} of {tuple(x.shape[1:])}, grid {G}, factors {f}, source "
                                 f"{src}: three values each")
        planes = Cc if want_prob else 1
        if min(src) < 1 or max(src) > 32767 or planes * math.prod(src) >= 2 ** 31:   # the outputs are not allocated for these
            raise _lib.EffqError(f"seg_probs_source: source grid {src}, {planes} planes: 1 to 32767 along an axis, "
                                 f"2^31 - 1 bytes at most")
        probs = torch.empty((Cc,) + src, dtype=torch.uint8, device=self.device) if want_prob else None
        unc = torch.empty(src, dtype=torch.uint8, device=self.device) if want_unc else None
        i3 = C.c_int * 3
        check(self.lib.effq_seg_probs_source(_ptr(x), Cc, i3(*(int(v) for v in x.shape[1:])), i3(*lo), i3(*G),
                                             (C.c_double * 3)(*f), i3(*src), code, _ptr(probs), _ptr(unc), self.stream),
              "effq_seg_probs_source")
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
        key = {"argmax": _lib.SEG_ARGMAX, "lits": _lib.SEG_ARGMAX, "sigmoid": _lib.SEG_SIGMOID,
               "brats": _lib.SEG_SIGMOID}.get(mode)
        if key is None:
            raise _lib.EffqError(f"seg_agreement: unknown mode {mode!r} (argmax or sigmoid)")
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
        if connectivity not in (6, 26):
            raise _lib.EffqError(f"cc_label: connectivity {connectivity}, 6 or 26")
        if P > 65535 or m.numel() >= 2 ** 31:
            raise _lib.EffqError(f"cc_label: {P} masks of {D * H * W} voxels (at most 65535 masks, 2^31 - 1 voxels in all)")
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
        if connectivity not in (6, 26):
            raise _lib.EffqError(f"cc_table: connectivity {connectivity}, 6 or 26")
        if P > 65535 or m.numel() >= 2 ** 31:
            raise _lib.EffqError(f"cc_table: {P} masks of {D * H * W} voxels (at most 65535 masks, 2^31 - 1 voxels in all)")

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
        if connectivity not in (6, 26):
            raise _lib.EffqError(f"label_clean: connectivity {connectivity}, 6 or 26")
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
        import numpy as np
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

    # -- the prep mission (prep.py) ---------------------------------------------------------------------------------
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
        if x.dtype != torch.float32 or not x.is_contiguous() or self._elsewhere(x) or x.numel() == 0:
            raise _lib.EffqError(f"prep_window: needs a contiguous float32 tensor on {self.device}")
        if not float(lo) <= float(hi):
            raise _lib.EffqError(f"prep_window: bounds {lo}, {hi}")
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
        if x.dtype != torch.float32 or not x.is_contiguous() or self._elsewhere(x) or x.numel() == 0:
            raise _lib.EffqError(f"prep_window_mask: needs a contiguous float32 tensor on {self.device}")
        mode = self._prep_mask("prep_window_mask", mask)
        if not float(lo) <= float(hi):
            raise _lib.EffqError(f"prep_window_mask: bounds {lo}, {hi}")
        check(self.lib.effq_prep_mask_window(_ptr(x), x.numel(), float(lo), float(hi), mode, self.stream),
              "effq_prep_mask_window")
        return x

    def prep_resample(self, x: torch.Tensor, factors, out_shape, nearest: bool = False) -> torch.Tensor:
        """N x D x H x W volumes on a grid of another spacing (effq_prep_resample): `factors` = target spacing / source
        spacing per axis, `out_shape` the output extents (prep.resample_extent).  float32 volumes are interpolated
        trilinearly; with `nearest` the volumes are uint8 labels and keep their values."""
        x, N, D, H, W = self._prep_volumes("prep_resample", x, torch.uint8 if nearest else torch.float32, limit_c=False)
        f = tuple(float(v) for v in factors)
        o = tuple(int(v) for v in out_shape)
        if len(f) != 3 or len(o) != 3 or not all(0.0 < v <= 1e6 for v in f) or min(o) < 1 or max(o) > 32767 or \
                N * o[0] * o[1] * o[2] >= 2 ** 31:
            raise _lib.EffqError(f"prep_resample: factors {f}, output extents {o}")
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
        f = tuple(float(v) for v in factors)
        o = tuple(int(v) for v in out_shape)
        if len(f) != 3 or len(o) != 3 or not all(0.0 < v <= 1e6 for v in f) or min(o) < 1 or max(o) > 32767 or \
                N * o[0] * o[1] * o[2] >= 2 ** 31:
            raise _lib.EffqError(f"prep_resample_cubic: factors {f}, output extents {o}")
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


_OPS = {}


def get_ops(device) -> HipOps:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = str(device)
    if key not in _OPS:
        _OPS[key] = HipOps(device)
    return _OPS[key]
