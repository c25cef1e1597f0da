"""Time effq_prep_joint_hist on the device at a BraTS-sized pair: the figures of DESIGN section 29.

    python scripts/time_prep_register.py [--reps 20] [--lib PATH]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/time_prep_register.py --reps 3

Per sample stride 4, 2, 1: the median time of one launch with the 13 candidates of a pattern-search step around a small
rigid move, on a smooth volume (the case of the search) and on a constant one (every sample in one bin: the worst case of
the LDS adds); one effq_prep_align call at the same output for scale; and the wall time of one whole registration.
`--lib` loads another build of the library, to set a variant of the kernel against the shipped one."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd import _lib  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=20)
p.add_argument("--lib", default=None)
args = p.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
from efficientq_amd import ops_align, ops_register, register as G  # noqa: E402
from efficientq_amd.hip_ops import get_ops  # noqa: E402

DEV = "cuda:0"
SHAPE = (240, 240, 155)
ops = get_ops(DEV)
EYE = np.eye(4)


def smooth_volume(seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 1, 12, 12, 8), generator=g)
    return (torch.nn.functional.interpolate(low, size=SHAPE, mode="trilinear", align_corners=True)[0, 0] * 900 + 100) \
        .contiguous().to(DEV)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


fixed, moving = smooth_volume(1), smooth_volume(2)
theta = (1.0, -0.5, 0.8, 0.01, -0.02, 0.015)
ms = np.stack([G.rigid_matrix("s", "m", EYE, EYE, SHAPE, t) for t in G.candidates(theta, 0.5, 0.004)])
fbin = ops_register.prep_bins(ops, fixed, 100.0, 32 / 900.0)
flat = torch.full(SHAPE, 500.0, device=DEV)
print(f"library {_lib.LIB_PATH}")
for s in (4, 2, 1):
    for what, mov in (("smooth", moving), ("constant", flat)):
        t = timed(lambda: ops_register.prep_joint_hist(ops, fbin, mov, ms, 100.0, 32 / 900.0, (s, s, s)))
        print(f"joint_hist K = 13 stride {s} {what}: {t:.3f} ms")
print(f"prep_align, one candidate: {timed(lambda: ops_align.prep_align(ops, moving, ms[0], SHAPE)):.3f} ms")
t0 = time.time()
ref = G.Reference(ops, "s", "ref", fixed, EYE, "all")
warped, _ = ops_align.prep_align(ops, 1100.0 - fixed, G.rigid_matrix("s", "m", EYE, EYE, SHAPE, theta), SHAPE)
torch.cuda.synchronize()
t1 = time.time()
got = G.register_rigid(ops, ref, "m", warped, EYE)
print(f"reference levels {[s for s, _ in ref.levels]} in {t1 - t0:.2f} s; one registration: {time.time() - t1:.2f} s, "
      f"{got.evals} launches, converged {got.converged}, NMI {got.nmi_before:.3f} -> {got.nmi_after:.3f}, theta {got.theta}")
