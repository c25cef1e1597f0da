"""What every group of wrappers shares: the per-device handle with its streams and library workspaces, and the two
argument helpers.  ``hip_ops.HipOps`` is composed from the groups (``ops_window``, ``ops_seg``, ``ops_prep``) and holds
the calibration wrappers itself."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import check


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(i) for i in v)


class OpsBase:
    """The handle itself: device, library, streams and workspaces (the plumbing of every wrapper group)."""

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
