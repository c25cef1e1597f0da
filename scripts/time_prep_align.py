"""Time whole calls of effq_prep_align on the device: the figures of DESIGN section 27.

    python scripts/time_prep_align.py [--reps 7] [--calls 200]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/time_prep_align.py --reps 1 --calls 5

One BraTS-size output, 155 x 240 x 240 at 1 mm, in both modes (trilinear on float32, nearest on uint8), from
  a  a 2 x coarser source (78 x 120 x 120 at 2 mm) turned 10 degrees about one axis around the volume's centre;
  b  a source with permuted axes: D and H swapped (W stays the innermost axis), and W outermost (every lane of a wave
     reads another source row);
and beside them, in the same process, effq_prep_resample to the same output size from the 2 x coarser source.  Per entry:
three warm-up calls, then `--reps` windows of `--calls` calls between a pair of device events; the median, the least
and the greatest time per call, and the bandwidth reached counting the source read once and the output written once."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd import prep  # noqa: E402
from efficientq_amd.hip_ops import get_ops  # noqa: E402
from efficientq_amd.ops_align import prep_align  # noqa: E402

OUT = (155, 240, 240)
COARSE = (78, 120, 120)


def centred(spacing, shape, rot, centre):
    """The affine rot diag(spacing) of a grid of `shape` whose middle lies at the world point `centre`."""
    a = np.eye(4)
    a[:3, :3] = rot @ np.diag(np.asarray(spacing, dtype=np.float64))
    a[:3, 3] = np.asarray(centre) - a[:3, :3] @ ((np.asarray(shape, dtype=np.float64) - 1.0) / 2.0)
    return a


def rotation(axis, degrees):
    t = np.deg2rad(degrees)
    i, j = [k for k in range(3) if k != axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    return r


def permutation(src_axis, shape):
    """Output axis p is source axis src_axis[p]: (the 3 x 4 matrix, the source shape)."""
    m = np.zeros((3, 4))
    src = [0, 0, 0]
    for p, a in enumerate(src_axis):
        m[a, p] = 1.0
        src[a] = shape[p]
    return m, tuple(src)


def timed(fn, reps, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / calls)
    return float(np.median(per)), min(per), max(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    dev = "cuda:0"
    ops = get_ops(dev)
    g = torch.Generator().manual_seed(0)
    ref = centred((1.0, 1.0, 1.0), OUT, np.eye(3), (0.0, 0.0, 0.0))
    turned = prep.align_matrix("timing", "rotated", centred((2.0, 2.0, 2.0), COARSE, rotation(0, 10.0), (0.0, 0.0, 0.0)), ref)
    swapped, n_swapped = permutation((1, 0, 2), OUT)
    outer, n_outer = permutation((2, 0, 1), OUT)
    sources = {}
    for shape in {COARSE, n_swapped, n_outer}:
        x = torch.rand(shape, generator=g).to(dev)
        sources[shape] = (x, (x * 255).to(torch.uint8))
    entries = []
    for name, m, shape in (("2 x coarser source turned 10 degrees", turned, COARSE), ("D and H swapped", swapped, n_swapped),
                           ("W outermost", outer, n_outer)):
        for k, mode in enumerate(("linear", "nearest")):
            x = sources[shape][k]
            y, inside = prep_align(ops, x, m, OUT, nearest=bool(k))
            print(f"{name}, {mode}: {int(inside.item()) / y.numel():.3f} of the output inside the field of view", flush=True)
            entries.append((f"prep_align {mode}, {name}", lambda x=x, m=m, k=k: prep_align(ops, x, m, OUT, nearest=bool(k)),
                            x.numel() * x.element_size() + y.numel() * y.element_size()))
    for k, mode in enumerate(("linear", "nearest")):
        x = sources[COARSE][k][None]
        entries.append((f"prep_resample {mode}, 2 x coarser source",
                        lambda x=x, k=k: ops.prep_resample(x, (0.5, 0.5, 0.5), OUT, nearest=bool(k)),
                        (x.numel() + int(np.prod(OUT))) * x.element_size()))
    for rnd in range(2):                    # twice: the spread between rounds is the noise of the figures
        for name, fn, nbytes in entries:
            med, lo, hi = timed(fn, args.reps, args.calls)
            print(f"round {rnd}: {name}: median {med:.3f} ms, least {lo:.3f}, greatest {hi:.3f}; "
                  f"{nbytes / med / 1e6:.0f} GB/s", flush=True)


if __name__ == "__main__":
    main()
