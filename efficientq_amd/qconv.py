"""Quantised Conv3d modules with the reference's class contract, computing on MI355X.

``PTQConv`` mirrors the reference base class (src/models/PTQConv.py:11-174): same
constructor, parameters (``weight``, ``bias``, 0-dim ``alpha_act``/``alpha_w``), mode
setters, ``forward`` dispatch, ``store_int_weight``/``restore_fp_weight``.
``EfficientQConvHIP`` mirrors ``EfficientQConv.ptq`` (src/models/EfficientQConv.py:33-166):
the layer-wise ADMM calibration, with every tensor computation issued through the C-ABI
library (``hip_ops``).  torch supplies memory, streams and the collective only.

Both class names contain ``QConv`` because the reference finds quantised layers by
class-name substring (src/models/model_blk.py:26-34).
"""
from __future__ import annotations

import math
import os
import time
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import hip_ops
from .hip_ops import from_ndhwc, make_geom, to_ndhwc

# ADMM constants are constructor constants in the reference (EfficientQConv.py:23-26)
LWQ_ITER, LWQ_RHO, LWQ_RHO_MAX, LWQ_ETA, RHO_PERIOD = 200, 10.0, 1000.0, 1.0, 50
EXACT_INT_DEFAULT = os.environ.get("EFFQ_EXACT_INT", "1") != "0"
# per-iteration losses from the unweighted Gram system (effq_gram_loss) for layers with n = k^3 c1 + 1 up to this size
GRAM_LOSS_DEFAULT = os.environ.get("EFFQ_GRAM_LOSS", "1") != "0"
GRAM_LOSS_MAX_N = 1729
# wide layers: the quadratic form on the i8 matrix cores up to this system size: measured per calibration, BraTS
# (n = 3457, 6913) 674 -> 657 ms with it; LiTS with its 512-channel layers (n = 13825) included 2110 -> 2169 ms (5.4 ms
# per group of 8 iterates beside a chain that is itself slowed by three concurrent 57 ms inverses), so those keep the
# integer conv pass
GRAM_LOSS_I8_MAX_N = 8000


def get_ops(device):
    """Indirection point: tests substitute a CPU stand-in built on the oracle here."""
    return hip_ops.get_ops(device)


def _call_if(ops, name, *args):
    """ops.<name>(*args) where the backend has that entry point, else False (the CPU stand-ins of the tests lack the
    optional kernels and the questions about them)."""
    fn = getattr(ops, name, None)
    return fn(*args) if fn is not None else False


class LayerPaths(NamedTuple):
    """The kernels one layer's calibration takes: layer_paths() chooses them, after() applies what only a call tells."""
    conv: Optional[str]      # integer family of the loss conv: None (the fp32 conv), "i8", "i8s" (direct gather)
    gram_i8: bool            # the Gram system from exact integer sums (else ops.gram)
    losses: Optional[str]    # the 200 losses: None (the loss conv), "gram_f64", "gram_i8" or "gram_f64_fp_input"
    want_idx: bool           # the level ids of the quantised input are needed
    fwd_i8: bool             # the final forward runs on the i8 matrix cores

    @property
    def loss_kind(self) -> int:
        return {None: 0, "i8": 1, "i8s": 2}[self.conv]

    def after(self, att_classes_ok: bool = True, planes_ok: bool = True) -> "LayerPaths":
        """att_classes() returned None (more distinct weights than the integer Gram kernel takes): the fp32 Gram system,
        no losses from it, level ids - and with them the i8 forward - only for an integer conv.  gram_loss_i8_planes()
        returned None (entries beyond its planes): the losses come from the loss conv again, nothing else changes."""
        p = self
        if p.gram_i8 and not att_classes_ok:
            p = p._replace(gram_i8=False, losses=None, want_idx=p.conv is not None,
                           fwd_i8=p.fwd_i8 and p.conv is not None)
        return p._replace(losses=None) if p.losses == "gram_i8" and not planes_ok else p


def layer_paths(ops, geom, act_levels, w_levels, has_bias, c2, n_sys, voxels, *, q_act, act_inited, exact_int,
                channel_wise, gram_loss_enabled, gram_loss_max_n, gram_loss_i8_max_n) -> LayerPaths:
    """The paths of a layer with n_sys = k^3 c1 (+ 1) unknowns and `voxels` output voxels per output channel, from its
    arguments alone; `ops` only answers what it supports."""
    int_ok = bool(q_act and not act_inited and exact_int)      # the level ids of an input quantised by a scale fitted here
    conv = None
    # channel mode: the integer conv losses and the i8 forward fold ONE weight scale into their arithmetic - off; the
    # integer Gram accumulation and the fp64 Gram loss (kind 4) take G as fp32 values and stay
    if int_ok and not channel_wise:
        # exact-integer evaluation of the 200 per-iteration losses (north_star's "int-simulated" forward)
        if _call_if(ops, "conv_i8_supported", geom, act_levels, w_levels):
            conv = "i8"
        # ... through the direct-gather kernel for short-K layers and the 256-level first/last layers
        elif _call_if(ops, "conv_i8s_supported", geom, act_levels, w_levels):
            conv = "i8s"
    # exact-integer evaluation of the Gram system too (exact integer sums, weights applied per attention class)
    gram_i8 = bool(int_ok and _call_if(ops, "gram_i8_supported", geom, act_levels))
    # Losses of the 200 iterates from the unweighted Gram system of the same integer pass (effq_gram_loss) instead of
    # 200 passes over the voxels, where the voxel count is far above n = k^3 c1 + 1 (the conv is cheaper on the small
    # volumes of the wide layers)
    many_voxels = n_sys <= gram_loss_max_n and voxels >= 8 * n_sys
    losses = None
    if gram_i8 and gram_loss_enabled:
        if many_voxels and hasattr(ops, "gram_loss"):
            losses = "gram_f64"
        # ... and on the wide layers (n above GRAM_LOSS_MAX_N: the fp64 evaluation would cost more than the conv pass)
        # with the quadratic form on the i8 matrix cores: both of its factors are small integers there (effq_gram_loss_i8)
        elif (not channel_wise and gram_loss_max_n < n_sys <= gram_loss_i8_max_n and
              _call_if(ops, "gram_loss_i8_supported", c2, n_sys, has_bias, w_levels)):
            losses = "gram_i8"
    # full-precision input (first conv, classifier: quirk Q14): the same 200 losses from an fp64 Gram system
    elif (not q_act and gram_loss_enabled and exact_int and many_voxels and
          _call_if(ops, "gram_f64_supported", geom, has_bias)):
        losses = "gram_f64_fp_input"
    want_idx = conv is not None or gram_i8
    # the final forward on the i8 matrix cores where the level ids of the input are at hand and the shape has a kernel
    # (32 -> 32 and 64 -> 64 channels at 3^3: the layers with the most voxels): an exact integer contraction + one
    # multiply-add per output, HBM-bound, instead of the f32 conv (2.6 -> 0.3 ms at 16 x 64^3 voxels)
    fwd_i8 = bool(int_ok and want_idx and not channel_wise and
                  _call_if(ops, "conv_i8_out_supported", geom, act_levels, w_levels))
    return LayerPaths(conv, gram_i8, losses, want_idx, fwd_i8)


class SumReducer:
    """Data-parallel SUM over calibration-volume shards (RCCL all-reduce; identity on one rank)."""

    calls = 0          # collectives issued by this process (tests, bench)

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist = dist
        # EFFQ_DP_FORCE=1: run the collectives even on one rank (exercises the RCCL path on a single GPU)
        force = os.environ.get("EFFQ_DP_FORCE", "0") == "1"
        self.on = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force)
        self.group = group
        self.direct = None
        if self.on and dist.get_backend(group) == "nccl":
            # RCCL called through its C ABI on the stream the kernels run on (rccl.py): no hop to the process group's
            # stream and back around every one of the ~50 tiny all-reduces of a layer.  EFFQ_RCCL_DIRECT=0: torch's path
            from . import rccl
            self.direct = rccl.get_comm(group)

    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        if self.on:
            SumReducer.calls += 1
            if t.is_cuda and self.direct is not None and t.is_contiguous():
                self.direct.all_reduce_sum_(t)
            elif t.is_cuda and self.dist.get_backend(self.group) == "gloo":
                # rehearsal mode (several ranks on ONE GPU, where RCCL refuses duplicate devices):
                # stage through the host; the product backend is "nccl" (= RCCL over xGMI)
                h = t.cpu()
                self.dist.all_reduce(h, op=self.dist.ReduceOp.SUM, group=self.group)
                t.copy_(h)
            else:
                self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t

    def all_gather(self, t: torch.Tensor) -> torch.Tensor:
        """Rank-major concatenation of every rank's `t` (same length on every rank)."""
        if not self.on:
            return t
        SumReducer.calls += 1
        if t.is_cuda and self.direct is not None and t.is_contiguous():
            return self.direct.all_gather(t)
        world = self.dist.get_world_size(self.group)
        if t.is_cuda and self.dist.get_backend(self.group) == "gloo":
            h = t.cpu()
            parts = [torch.empty_like(h) for _ in range(world)]
            self.dist.all_gather(parts, h, group=self.group)
            return torch.cat(parts).to(t.device)
        parts = [torch.empty_like(t) for _ in range(world)]
        self.dist.all_gather(parts, t.contiguous(), group=self.group)
        return torch.cat(parts)

    @property
    def world(self) -> int:
        return self.dist.get_world_size(self.group) if self.on else 1

    @property
    def rank(self) -> int:
        return self.dist.get_rank(self.group) if self.on else 0

    def __bool__(self):
        return self.on


class _QuantConvFn(torch.autograd.Function):
    """Quantised forward of a PTQConv with gradients for tune_activation_range (ptqer.py:238-272): the forward is the
    fused act-quant conv kernel; the backward is the same conv kernel on the output gradient (flipped, transposed
    weights) followed by the straight-through backward of the activation quantiser.  Weights take no gradient."""

    @staticmethod
    def forward(ctx, x, alpha, mod):
        ctx.mod = mod
        ctx.save_for_backward(x, alpha)
        # (a fresh tensor, not the permuted view _conv returns: the next block's in-place ReLU writes into it)
        return mod._conv(x, mod.q_act).clone(memory_format=torch.preserve_format)

    @staticmethod
    def backward(ctx, g):
        mod = ctx.mod
        x, alpha = ctx.saved_tensors
        need_x = ctx.needs_input_grad[0]
        if not need_x and not mod.q_act:
            return None, None, None
        gq = mod._dgrad(g)
        if not mod.q_act:
            return gq, None, None
        ops = get_ops(g.device)
        gx, ga = ops.act_quant_backward(to_ndhwc(x.detach()), alpha.detach(), mod.qlvl_act, to_ndhwc(gq), want_gx=need_x)
        return (from_ndhwc(gx) if need_x else None), ga.to(alpha.dtype).reshape(alpha.shape), None


class PTQConv(nn.Conv3d):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, q_weight=True, qlvl=8, q_act=True, qlvl_act=8, **kwQ):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)
        if self.dilation != (1, 1, 1) or self.groups != 1:
            # the reference's solver ignores both (solver.py:86-111); both shipped configs use 1
            raise NotImplementedError("dilation/groups other than 1 are outside the calibrated path")
        self.conv_param = dict(stride=stride, padding=padding, dilation=dilation, groups=groups)
        self.q_act, self.q_weight = q_act, q_weight
        self.qlvl_w, self.qlvl_act = qlvl, qlvl_act
        self.kwQ = kwQ
        self.alpha_act = nn.Parameter(torch.tensor(1.))
        # lwq_channel_wise (not in the reference): one weight scale per output channel, alpha_w of shape (c2, 1, 1, 1)
        self.channel_wise = bool(kwQ.get('lwq_channel_wise', False))
        self.alpha_w = nn.Parameter(torch.ones(out_channels, 1, 1, 1) if self.channel_wise else torch.tensor(1.))
        self.output_fp = None            # FP target, set by the forward hook
        self.name = None
        self.snap_dir = kwQ.get('snap_dir', None)
        self.w_backup = self.b_backup = None
        self._act_inited = False
        self.set_fp()

    # ---- mode flags (PTQConv.py:50-72) --------------------------------------------------------
    def _mode(self, fp=False, quantizing=False, quantized=False, init_act=False):
        self._fp, self._quantizing, self._quantized, self._init_act = fp, quantizing, quantized, init_act

    def set_fp(self):
        self._mode(fp=True)

    def set_quantizing(self):
        self._mode(quantizing=True)

    def set_quantized(self):
        self._mode(quantized=True)

    def set_init_act(self):
        self._mode(init_act=True)

    def qweight_init_iter(self):
        pass

    def qparam_init(self):
        pass

    def perform_quantization(self):
        pass

    def backup_weight(self):
        self.w_backup = self.weight.data.cpu().clone()
        if self.bias is not None:
            self.b_backup = self.bias.data.cpu().clone()

    # ---- device helpers ------------------------------------------------------------------------
    def _geom(self, x):
        return make_geom(x.shape, self.out_channels, self.kernel_size, self.stride, self.padding)

    def _conv(self, x, quantize_act: bool):
        """conv3d (optionally with the fp32 activation quant-dequant fused into the tile load)."""
        ops = get_ops(x.device)
        out, _ = ops.conv_step(to_ndhwc(x.detach()), self.weight.data, None if self.bias is None else self.bias.data,
                               self._geom(x), act_alpha=self.alpha_act.data if quantize_act else None,
                               act_levels=self.qlvl_act if quantize_act else 0, want_out=True)
        return from_ndhwc(out)

    def _dgrad(self, g):
        """Gradient of the conv w.r.t. its input: the conv kernel on g with flipped, transposed weights.  Stride 1 and
        "same" padding (2 p = k - 1 on every axis) only: there the gradient conv has the forward's own padding."""
        if self.stride != (1, 1, 1):
            raise NotImplementedError("input gradient of a strided conv is not needed on the calibrated path")
        if any(2 * p != k - 1 for p, k in zip(self.padding, self.kernel_size)):
            raise NotImplementedError(f"input gradient needs 'same' padding (2 * padding == kernel_size - 1), got "
                                      f"kernel_size {tuple(self.kernel_size)} with padding {tuple(self.padding)}")
        ops = get_ops(g.device)
        # formed on every backward: the weights are written through .data, which leaves no trace a cache could key on
        # (neither _version nor, with the caching allocator, the address), and the tensor is small beside the conv
        wt = self.weight.data.flip(2, 3, 4).transpose(0, 1).contiguous()
        geom = make_geom(g.shape, self.in_channels, self.kernel_size, self.stride, self.padding)
        out, _ = ops.conv_step(to_ndhwc(g.detach()), wt, None, geom, want_out=True)
        return from_ndhwc(out)

    def _quantize_act(self, x):
        """discretize(x/alpha_act, L, 0, 1) * alpha_act in fp32 (PTQConv.py:114-116)."""
        ops = get_ops(x.device)
        return from_ndhwc(ops.quant_dequant_f32(to_ndhwc(x.detach()), self.alpha_act.data, self.qlvl_act, 0.0, 1.0))

    def _quantize_w(self):
        ops = get_ops(self.weight.device)
        return ops.quant_dequant_f32(self.weight.data, self.alpha_w.data, self.qlvl_w, -1.0, 1.0)

    def init_alpha_act(self, x):
        """PTQConv.py:74-78."""
        ops = get_ops(x.device)
        xn = to_ndhwc(x.detach())
        red = SumReducer()
        if self.qlvl_act < 2:
            # "W,-1" layers (full-precision activations, quirk Q14) still pass through here in the init pass: with
            # num_lvl = -1 project_by_iter's loop never runs (max_iter = -100), so a = mean|x|, and discretize works with
            # delta = 1/(-2): values land on {0, 0.5, 1} - the arithmetic of 3 levels (layer_helper.py:25-37,50-66)
            s0 = ops.abs_sum(xn)
            if red:
                red(s0)
            st = ops.new_fp_state()
            st[0] = s0[0] / s0[1]
            a, levels = st[0].item(), 3
        else:
            a, _, st = ops.fit_scale(xn, self.qlvl_act, 0.0, 1.0, reducer=red or None)
            levels = self.qlvl_act
        self.alpha_act.data = torch.tensor(a, device=x.device)
        self._act_inited = True
        y, _, _ = ops.quant_dequant_f64path(xn, st, levels, 0.0, 1.0)
        return from_ndhwc(y)

    def ptq(self, x):
        raise NotImplementedError

    # ---- storage formats (PTQConv.py:125-152) -----------------------------------------------
    def store_int_weight(self):
        """Level ids as uint8 (<=256 levels) / int32, for storage only.  Uses the saved alpha_w,
        which is the LAST iterate's scale while weight is the BEST iterate's (quirk Q6).
        Channel mode: alpha_w (c2, 1, 1, 1) is the best iterate's, so the ids are exact; a row with scale 0 stores
        level (L-1)//2."""
        a = self.alpha_w.data
        delta = 2 / (self.qlvl_w - 1)
        if self.channel_wise:
            w_int = self._channel_ids(self.weight.data, a, self.qlvl_w)
        else:
            b = self.weight.data / a
            w_int = torch.round((b + 1) / delta)
        w_int = w_int.to(torch.uint8) if self.qlvl_w <= 256 else w_int.to(torch.int32)
        self.weight.requires_grad = False
        self.weight.data = w_int.data.cpu()

    def restore_fp_weight(self):
        delta = 2 / (self.qlvl_w - 1)
        if self.channel_wise:
            self.weight.data = self._channel_weight(self.weight.data, self.alpha_w.data, self.qlvl_w)
            return
        b = self.weight.data.float() * delta - 1
        self.weight.data = self.alpha_w.data * b

    @staticmethod
    def _channel_ids(w, a, levels):
        """Level ids of weights on per-row grids alpha_c * (2 j / (L-1) - 1); rows with alpha_c = 0 -> (L-1)//2."""
        a = a.to(w.device).reshape(-1, *([1] * (w.dim() - 1)))
        delta = 2 / (levels - 1)
        zero = a == 0
        ids = torch.round((w / torch.where(zero, torch.ones_like(a), a) + 1) / delta)
        return torch.where(zero, torch.full_like(ids, float((levels - 1) // 2)), ids)

    @staticmethod
    def _channel_weight(ids, a, levels):
        """Inverse of _channel_ids with the calibrator's arithmetic: b = fp32(id * d - 1 in fp64), w = fp32(alpha_c) * b
        (the same bits as the calibrated weights); rows with alpha_c = 0 -> +0."""
        a = a.to(ids.device).reshape(-1, *([1] * (ids.dim() - 1))).float()
        b = (ids.double() * (2 / (levels - 1)) - 1).float()
        return torch.where(a == 0, torch.zeros_like(b), a * b)

    # ---- bit-packed storage (row f2; the reference keeps one uint8 per weight) ------------------
    def export_packed_weight(self):
        """Level ids of the quantised weight packed at 1/2/4/8 bits each: dict(data, n, bits, shape, alpha_w, levels).
        Same level ids as store_int_weight(); the module is left untouched."""
        ops = get_ops(self.weight.device)
        delta = 2 / (self.qlvl_w - 1)
        if self.channel_wise:         # alpha_w travels as a list of c2 scales, flagged channel_wise=True
            ids = self._channel_ids(self.weight.data, self.alpha_w.data, self.qlvl_w)
            ids = ids.to(torch.uint8).contiguous().reshape(-1)
            bits = ops.storage_bits(self.qlvl_w)
            return dict(data=ops.pack_levels(ids, bits).cpu(), n=int(ids.numel()), bits=bits,
                        shape=tuple(self.weight.shape), alpha_w=self.alpha_w.data.reshape(-1).tolist(),
                        levels=int(self.qlvl_w), channel_wise=True)
        ids = torch.round((self.weight.data / self.alpha_w.data + 1) / delta).to(torch.uint8).contiguous().reshape(-1)
        bits = ops.storage_bits(self.qlvl_w)
        return dict(data=ops.pack_levels(ids, bits).cpu(), n=int(ids.numel()), bits=bits,
                    shape=tuple(self.weight.shape), alpha_w=float(self.alpha_w.data), levels=int(self.qlvl_w))

    def import_packed_weight(self, blob):
        """Inverse of export_packed_weight(): weight = alpha_w * (2*id/(L-1) - 1), like restore_fp_weight()."""
        ops = get_ops(self.weight.device)
        ids = ops.unpack_levels(blob["data"].to(self.weight.device), blob["n"], blob["bits"])
        if blob.get("channel_wise", False):
            a = torch.tensor(blob["alpha_w"], dtype=self.weight.dtype, device=self.weight.device)
            self.alpha_w.data = a.reshape(-1, 1, 1, 1)
            self.weight.data = self._channel_weight(ids.reshape(blob["shape"]), a, blob["levels"])
            return
        delta = 2 / (blob["levels"] - 1)
        self.alpha_w.data = torch.tensor(blob["alpha_w"], dtype=self.weight.dtype, device=self.weight.device)
        self.weight.data = (self.alpha_w.data * (ids.float() * delta - 1)).reshape(blob["shape"])

    # ---- forward dispatch (PTQConv.py:154-174) ----------------------------------------------
    def forward(self, x):
        if self._fp:
            return self._conv(x, False)
        if self._quantizing:
            self._ptq_out = None
            self.ptq(x)
            out, self._ptq_out = getattr(self, "_ptq_out", None), None
            return from_ndhwc(out) if out is not None else self._conv(x, self.q_act)
        if self._quantized:
            if torch.is_grad_enabled() and (self.alpha_act.requires_grad or x.requires_grad):
                return _QuantConvFn.apply(x, self.alpha_act, self)      # tune_activation_range (row f3)
            return self._conv(x, self.q_act)
        if self._init_act:
            qact = self.init_alpha_act(x)
            return self._conv(qact, False)
        raise RuntimeError(f"Unknown FP/Quant setting: FP={self._fp}, "
                           f"Quantizing={self._quantizing}, Quantized={self._quantized}")


class EfficientQConvHIP(PTQConv):
    """Layer-wise ADMM calibrator (EfficientQConv.py:13-166) on the HIP library.

    ``lwq_channel_wise=True`` (not in the reference) fits one weight scale per output channel: the projection of every
    ADMM iteration runs project_by_iter on each output row of w* + dual (effq_fixed_point_channels_proj); prox solve,
    dual update and the loss from the fp32 conv (or the fp64 Gram system) are unchanged.  The integer conv losses and
    the i8 forward, which fold one scalar scale into their arithmetic, are not used.  ``alpha_w`` is then a
    (c2, 1, 1, 1) parameter holding the BEST iterate's scales - unlike the per-tensor quirk Q6, which keeps the last
    iterate's scale - so the saved weights lie exactly on their rows' grids.  A row whose values are all zero gets
    scale 0 and weights 0."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, q_weight=True, qlvl=8, q_act=True, qlvl_act=8, **kwQ):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         q_weight, qlvl, q_act, qlvl_act, **kwQ)
        self.lwq_iter, self.lwq_rho, self.lwq_rho_max, self.lwq_eta = LWQ_ITER, LWQ_RHO, LWQ_RHO_MAX, LWQ_ETA
        self.lwq_fold_bn = True
        self.lwq_verbose = kwQ.get('lwq_verbose', False)
        self.mask_pyramid = None
        self.layer_loss = None
        self.last_trace = None          # diagnostics of the last calibration (not in the reference)
        self.lwq_trace = kwQ.get('lwq_trace', False)   # record the per-iteration loss (one host sync each)
        # evaluate the per-iteration losses on the i8 matrix cores (exact int32 accumulation) where supported
        self.lwq_exact_int = kwQ.get('lwq_exact_int', EXACT_INT_DEFAULT)
        # evaluate the loss of iteration i on a second stream while the chain computes iteration i+1
        self.lwq_overlap_loss = kwQ.get('lwq_overlap_loss', True)

    @staticmethod
    def _std(m: torch.Tensor) -> float:
        """Unbiased std from [sum, sumsq, n] (Tensor.std(), EfficientQConv.py:46,48)."""
        s, ss, n = m.tolist() if hasattr(m, "tolist") else m
        return math.sqrt(max(ss - s * s / n, 0.0) / (n - 1))

    def ptq(self, x):
        c = self._layer_inputs(x)
        ops, red = c.ops, c.red
        rho_scale, y_dim, att, sx, syy_local = self._statistics(c)
        paths = layer_paths(ops, c.geom, self.qlvl_act, self.qlvl_w, c.has_b, c.c2, c.n_sys, c.voxels, q_act=self.q_act,
                            act_inited=self._act_inited, exact_int=self.lwq_exact_int, channel_wise=self.channel_wise,
                            gram_loss_enabled=GRAM_LOSS_DEFAULT, gram_loss_max_n=GRAM_LOSS_MAX_N,
                            gram_loss_i8_max_n=GRAM_LOSS_I8_MAX_N)
        att_cls = ops.att_classes(att) if paths.gram_i8 else None
        paths = paths.after(att_classes_ok=att_cls is not None)
        xq, xidx, act_iters = self._quantise_input(c, sx, paths.want_idx)
        rho = self.lwq_rho * rho_scale                                    # (:74-76)
        rho_m = self.lwq_rho_max * rho_scale
        eta = self.lwq_eta * rho_scale
        A0, B0, loss_gram, paths = self._gram_system(c, paths, xq, xidx, att, att_cls, syy_local)
        t_loop0 = time.perf_counter()
        run = self._admm_run(c, paths, A0, B0, xq, xidx, loss_gram, rho, rho_m, eta)
        t_enq = time.perf_counter() - t_loop0     # host time to enqueue the 200 iterations (diagnostic)
        red(run.hist)
        best_G, best_b, best = ops.admm_select_best(run)
        fin = self._final_forward(c, paths, run, best, best_G, best_b, xq, xidx, att)
        red(fin)
        info = ops.admm_read(run, best, extra=fin)                         # ONE host sync for the loop and the final loss
        t_loop = time.perf_counter() - t_loop0
        self._print_progress(run, info["hist"], rho, rho_m, eta, y_dim)
        self._raise_on_error(ops, info)
        _call_if(ops, "release_retired")     # every stream was joined and the host has synchronised
        self._commit(c, best_G, best_b, info["alpha_w"])
        fin_h, best_h, numel = info["extra"], info["best"], y_dim * 1.0
        lossf = (fin_h[1] if att is not None else fin_h[0]) / numel
        if self.layer_loss is not None:
            self.layer_loss.append(f'{self.name:45s}:{lossf}')
        self.last_trace = dict(rho_scale=rho_scale, best_iter=int(best_h[1]), best_mse=best_h[0] / numel,
                               final_mse=fin_h[0] / numel, layer_loss=lossf, act_iters=act_iters,
                               w_iters=info["w_iters"], alpha_w=info["alpha_w"],
                               loss_history=[h / numel for h in info["hist"]],
                               exact_int=paths.conv is not None or paths.losses is not None, exact_gram=paths.gram_i8,
                               gram_loss=paths.losses is not None, host_enqueue_s=t_enq, admm_loop_s=t_loop,
                               channel_wise=self.channel_wise, paths=paths._asdict())

    def _layer_inputs(self, x):
        """What the steps of ptq read and none of them changes; n_sys = k^3 c1 (+ 1) unknowns per output channel."""
        ops, red, dev, c2, has_b = get_ops(x.device), SumReducer(), x.device, self.out_channels, self.bias is not None
        xn = to_ndhwc(x.detach())
        yn = to_ndhwc(self.output_fp.detach().to(dev))
        geom = self._geom(x)
        W0 = self.weight.data.contiguous()
        b0 = self.bias.data.contiguous() if has_b else None
        return SimpleNamespace(ops=ops, red=red, dev=dev, x=x, xn=xn, yn=yn, geom=geom, W0=W0, b0=b0, has_b=has_b, c2=c2,
                               n_sys=W0.numel() // c2 + int(has_b), voxels=yn.numel() // c2)

    def _statistics(self, c):
        """(rho_scale, y_dim, att, sx, syy_local): the layer's moments, packed into one all-reduce and one host read."""
        ops, red = c.ops, c.red
        # rho_scale = max(numel(y)*std(y) / (numel(W)*std(W)), 1) [* mean(att)]     (EfficientQConv.py:43-49, :51-62)
        # the three moment triples are enqueued first and read by ONE device->host copy (each read empties the queue:
        # the device idles for the round trip)
        my = ops.moments(c.yn)
        syy_local = my[1:2].clone()           # sum y^2 over THIS rank's voxels (the loss from the Gram system adds it)
        mw = ops.moments(c.W0)
        att = None
        if self.lwq_verbose:
            print(f'Calibrating {self.name}')
        if self.mask_pyramid:
            for mask in self.mask_pyramid:
                if tuple(mask.shape[1:]) == tuple(self.output_fp.shape[2:]):
                    att = mask.to(c.dev).contiguous()
                    break
        ma = ops.moments(att) if att is not None else None
        # data-parallel: the layer's three statistics triples - targets, attention weights, sum|x| of the input for the
        # start of its scale fit - travel as ONE message (they were three)
        fit_here = bool(self.q_act and not self._act_inited)
        sx = ops.abs_sum(c.xn) if (fit_here and red and hasattr(ops, "abs_sum")) else None
        if red:
            parts = [t for t in (my, ma, sx) if t is not None]
            pack = red(torch.cat(parts))
            off = 0
            for t in parts:
                t.copy_(pack[off:off + t.numel()])
                off += t.numel()
        mh = torch.cat([my, mw] + ([ma] if ma is not None else [])).tolist()
        y_dim = mh[2]
        rho_scale = max(y_dim * self._std(mh[0:3]) / (c.W0.numel() * self._std(mh[3:6])), 1.0)
        if ma is not None:
            rho_scale *= mh[6] / mh[8]
        return rho_scale, y_dim, att, sx, syy_local

    def _quantise_input(self, c, sx, want_idx):
        """(xq, xidx, act_iters): the input as the loop sees it (:64-72); fits alpha_act where it is not initialised."""
        if not self.q_act:
            return c.xn, None, 0
        if self._act_inited:
            return to_ndhwc(self._quantize_act(c.x)), None, 0
        kw_fit = dict(abs_sums=sx) if sx is not None else {}
        a_act, act_iters, st = c.ops.fit_scale(c.xn, self.qlvl_act, 0.0, 1.0, reducer=c.red or None,
                                               guess_iters=12 * self.qlvl_act, **kw_fit)
        self.alpha_act.data = torch.tensor(a_act, dtype=c.x.dtype, device=c.dev)
        xq, _, xidx = c.ops.quant_dequant_f64path(c.xn, st, self.qlvl_act, 0.0, 1.0, want_idx=want_idx)
        return xq, xidx, act_iters

    def _gram_system(self, c, paths, xq, xidx, att, att_cls, syy_local):
        """(A0, B0, loss_gram, paths): the Gram system, summed over the ranks, and the operands of the Gram losses."""
        ops, a_act, loss_gram = c.ops, self.alpha_act.data, None
        if paths.gram_i8 and paths.losses:
            A0, B0, Au, Bu = ops.gram_i8(xidx, att_cls, c.yn, c.geom, c.has_b, a_act, self.qlvl_act, unweighted=True)
            loss_gram = (Au, Bu, syy_local)
            if paths.losses == "gram_i8":
                planes = ops.gram_loss_i8_planes(Au, c.has_b, a_act, self.qlvl_act, c.voxels)
                paths = paths.after(planes_ok=planes is not None)
                loss_gram = (Au, Bu, syy_local, planes) if planes is not None else None
        elif paths.gram_i8:                                                # (:87-91, solver.py:282-314)
            A0, B0 = ops.gram_i8(xidx, att_cls, c.yn, c.geom, c.has_b, a_act, self.qlvl_act)
        else:
            A0, B0 = ops.gram(xq, att, c.yn, c.geom, c.has_b)
            if paths.losses:                                               # "gram_f64_fp_input"
                Au, Bu = ops.gram_f64(xq, c.yn, c.geom, c.has_b)
                loss_gram = (Au, Bu, syy_local)
        if c.red:                    # one message per layer: upper triangle of A0 + B0
            if hasattr(ops, "gram_reduce"):
                ops.gram_reduce(A0, B0, c.red)
            else:
                c.red(A0)
                c.red(B0)
        return A0, B0, loss_gram, paths

    def _admm_run(self, c, paths, A0, B0, xq, xidx, loss_gram, rho, rho_m, eta):
        # The 200 iterations (:99-144) are enqueued by ONE library call (effq_admm_run): the serial chain prox ->
        # scale fixed point -> projection/dual on this stream, the loss of iteration i (conv + MSE, used only to pick
        # the best iterate) on a second stream while the chain computes i+1, the inverses of A(rho) for the later rho
        # values (A changes only with rho: 4 inverses per layer, not 200 LU solves) on a third.  Per-iteration results
        # stay in rings, the squared errors in `hist`; the best iterate is selected afterwards - so the data-parallel
        # reduction of the 200 losses is ONE collective per layer.
        kw = dict(loss_gram=loss_gram) if loss_gram is not None else {}
        if self.channel_wise:
            kw['channel_wise'] = True     # effq_fixed_point_channels_proj: one scale per output row
        if self.lwq_verbose:
            kw['residuals'] = True        # the per-iteration residual norms of the reference's progress line (:114-127)
        return c.ops.admm_run(A0, B0, c.W0, c.b0, c.geom, c.yn, xq=xq, xidx=xidx, act_alpha=self.alpha_act.data,
                              act_levels=self.qlvl_act, loss_kind=paths.loss_kind, rho=rho, rho_max=rho_m, eta=eta,
                              iters=self.lwq_iter, period=RHO_PERIOD, levels=self.qlvl_w,
                              overlap=self.lwq_overlap_loss, **kw)

    def _final_forward(self, c, paths, run, best, best_G, best_b, xq, xidx, att):
        # (:161-166) the final loss - and, from the same pass, the layer's quantised output, which forward() hands to the
        # next layer right after this call (PTQConv.py:160-163 runs the same conv a second time): the fp32 activation
        # quant-dequant is fused into the tile load, exactly as in the quantised forward.  Enqueued BEFORE the layer's
        # one device->host read, which then carries its two sums as well.
        fuse = self.q_act and not self._act_inited
        if paths.fwd_i8:
            st_best = run.state_ring.index_select(0, best[1:2].to(torch.long)).reshape(-1)    # the best iterate's scale
            out, fin = c.ops.conv_forward_i8(xidx, best_G, best_b, c.geom, c.yn, att, self.alpha_act.data, self.qlvl_act,
                                             st_best, self.qlvl_w)
        else:
            out, fin = c.ops.conv_step(c.xn if fuse else xq, best_G, best_b, c.geom, c.yn, att,
                                       act_alpha=self.alpha_act.data if fuse else None,
                                       act_levels=self.qlvl_act if fuse else 0, want_out=True)
        self._ptq_out = out if (fuse or not self.q_act) else None
        return fin

    def _print_progress(self, run, hist, rho, rho_m, eta, y_dim):
        if not (self.lwq_verbose and getattr(run, "res", None) is not None):
            return
        # "print every 10 admm iters" (EfficientQConv.py:124-127), after the loop: the iterations are enqueued as a whole
        res, r_i = run.res.cpu(), rho
        for i in range(self.lwq_iter):
            if i % 10 == 0:
                print(f'ADMM iter {i + 1}: primal residual = {float(res[i, 0]) ** 0.5:.4f}, '
                      f'dual residual = {r_i * float(res[i, 1]) ** 0.5:.4f}, rho = {r_i:.4f}, eta = {eta:.4f}, '
                      f'loss = {hist[i] / (y_dim * 1.0):.7f}.')
            if i % RHO_PERIOD == 0:
                r_i = r_i * 2 if r_i * 2 <= rho_m else rho_m

    def _raise_on_error(self, ops, info):
        if info["err"] >= 1000:
            raise RuntimeError(f'{self.name}: the unweighted Gram system is not the integer system effq_gram_loss_i8 '
                               f'expects (flag {info["err"] // 1000})')
        if info["err"] == 0:
            return
        if info["err"] == 2:                                               # layer_helper.py:62-64
            where = ''
            if self.channel_wise:
                i_cap = next((i for i, w in enumerate(info["w_iters"]) if w >= 100 * self.qlvl_w), None)
                if i_cap is not None:
                    where = f' (output channel {info["w_iters_rows"][i_cap]}, ADMM iteration {i_cap})'
            raise RuntimeWarning(f'Exceed maximum iteration ({100 * self.qlvl_w}) for alpha optimization{where}')
        # state 3 = the grid barrier of the cooperative fixed point timed out (its workgroups were not co-resident):
        # its barrier words in the reduction workspace are left non-zero - clear them before reporting
        if hasattr(ops, "_red_ws"):
            ops._red_ws.zero_()
        raise RuntimeError(f'weight-scale fixed point did not finish (device state {info["err"]}: grid barrier '
                           f'time-out of the cooperative kernel)')

    def _commit(self, c, best_G, best_b, a_w):
        self.weight.data = best_G.reshape(self.weight.shape)               # (:147-158)
        if c.has_b:
            self.bias.data = best_b
        if self.channel_wise:
            # the BEST iterate's scales (not the last iterate's as in the per-tensor quirk Q6): the saved weights then lie
            # exactly on alpha_w's grids, and store_int_weight is exact
            self.alpha_w.data = torch.tensor(a_w, dtype=c.x.dtype, device=c.dev).reshape(c.c2, 1, 1, 1)
        else:
            self.alpha_w.data = torch.tensor(a_w, dtype=c.x.dtype, device=c.dev)   # LAST iterate's scale (quirk Q6)

    def compute_quant_error(self, output_fp, Qw, Qact):
        """EfficientQConv.py:168-172."""
        ops = get_ops(Qact.device)
        _, sq = ops.conv_step(to_ndhwc(Qact), Qw, None if self.bias is None else self.bias.data,
                              self._geom(Qact), to_ndhwc(output_fp))
        return sq[0].item() / output_fp.numel()
