"""Times of the local conditional random field on one 240 x 240 x 155 volume with four modalities:
effq_seg_crf at C = 3 in softmax and in sigmoid mode, T = 5 and T = 1 (the cost of one launch), at the radii 3 3 3 and,
for a W spacing of 2.5 mm, 3 3 2 (the rolled form of the kernel); one warm-up and then --repeat calls between device
events each; median with min and max, and the rate in voxel-neighbour pairs per second.

    python scripts/prof_seg_crf.py [--repeat 10]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd import crf, ops_crf                       # noqa: E402
from efficientq_amd.hip_ops import get_ops                    # noqa: E402


def times_ms(fn, repeat):
    fn()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    repeat = ap.parse_args().repeat
    ops = get_ops("cuda:0")
    shape, classes, mods = (240, 240, 155), 3, 4
    g = torch.Generator(device="cuda:0").manual_seed(0)
    z = torch.stack(torch.meshgrid(*[torch.linspace(-1, 1, n, device="cuda:0") for n in shape], indexing="ij"))
    x = torch.stack([(0.5 + 0.1 * m) * z.sum(0) + (z[1] * z[2] > 0.1 * m) for m in range(mods)]).float()
    x = (x + 0.2 * torch.randn(x.shape, generator=g, device="cuda:0")).contiguous()
    v = (4.0 * torch.randn((classes,) + shape, generator=g, device="cuda:0")).contiguous()
    need = C.c_size_t()
    assert ops.lib.effq_seg_crf_ws_bytes(classes, *shape, C.byref(need)) == 0
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda:0")
    out, changed = torch.empty_like(v), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    p = crf.DEFAULTS
    for spacing in ((1.0, 1.0, 1.0), (1.0, 1.0, 2.5)):     # radii 3 3 3: the unrolled row of pairs; 3 3 2: the rolled one
        radii = crf.radii(spacing, p)
        pairs = int(np.prod(shape)) * (int(np.prod([2 * r + 1 for r in radii])) - 1)
        print(f"{shape}, C {classes}, M {mods}, radii {radii}: {pairs / 1e9:.2f} G pairs per iteration, workspace "
              f"{need.value / 2 ** 20:.0f} MiB")
        for mode in ("softmax", "sigmoid"):
            for iters in (1, p.iters):
                def launch():                         # the launches alone: no read-back between the events
                    rc = ops.lib.effq_seg_crf(v.data_ptr(), classes, x.data_ptr(), mods, *shape, *spacing,
                                              ops_crf.MODES[mode], p.w_a, p.w_s, p.theta_p, p.theta_i, p.theta_s, iters, 0.0,
                                              out.data_ptr(), changed.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream)
                    assert rc == 0, rc
                med, lo, hi = times_ms(launch, repeat)
                print(f"{mode} T {iters}: {med:.2f} ms ({lo:.2f} - {hi:.2f}), {iters * pairs / med / 1e6:.1f} G pairs / s, "
                      f"{int(changed.cpu()[0])} voxels changed")


if __name__ == "__main__":
    main()
