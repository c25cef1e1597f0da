"""Time effq_seg_probs_source (HipOps.seg_probs_source) on the device beside effq_seg_labels_source: the cases of DESIGN
sections 15 and 20.

    python scripts/prof_seg_prob.py [--launches 20] [--classes 3]

The six shapes of scripts/prof_seg_source.py, source grids (SD, SH, SW) as the kernels take them.  Per case: random
logits of 4 N(0, 1) on the device; for the label kernel and for the probability kernel with the probabilities, the
uncertainty and both wanted, one warm-up launch and then `--launches` launches, each between a pair of device events;
the median, the least and the greatest are printed beside the bytes each pass must move (the logits once, its outputs
once).  The outputs are allocated by the ops inside the timed span, as in prof_seg_source.py and in the mission."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd.hip_ops import get_ops  # noqa: E402
from prof_seg_source import CASES  # noqa: E402


def timed(fn, launches):
    """(median, least, greatest) in ms of `launches` calls of fn after one warm-up, and what the last call returned."""
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(torch.cuda.current_stream())
        out = fn()
        t1.record(torch.cuda.current_stream())
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return (statistics.median(times), min(times), max(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--classes", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    ops = get_ops(dev)
    for name, src, f, box, rule, fuse in CASES:
        G = src if f is None else tuple(max(1, round(n / x)) for n, x in zip(src, f))
        pmin, ext = box if box is not None else ((0, 0, 0), G)
        logits = 4.0 * torch.randn((a.classes,) + tuple(ext), device=dev)
        mode = "argmax" if rule == "argmax" else "sigmoid"
        vox = src[0] * src[1] * src[2]
        read = logits.numel() * 4
        print(f"{name}: source (SD, SH, SW) = {src}, grid {tuple(G)}, box {tuple(ext)} at {tuple(pmin)}, C = {a.classes}",
              flush=True)
        runs = [(f"labels {rule}/{fuse}", vox, lambda: ops.seg_labels_source(logits, pmin, G, f, src, rule, fuse)),
                (f"probs {mode}", a.classes * vox, lambda: ops.seg_probs_source(logits, pmin, G, f, src, mode, True, False)),
                (f"unc {mode}", vox, lambda: ops.seg_probs_source(logits, pmin, G, f, src, mode, False, True)),
                (f"probs + unc {mode}", (a.classes + 1) * vox,
                 lambda: ops.seg_probs_source(logits, pmin, G, f, src, mode, True, True))]
        for what, written, fn in runs:
            (med, lo, hi), _ = timed(fn, a.launches)
            nbytes = read + written
            print(f"    {what}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of {a.launches}; writes "
                  f"{written / 1e6:.1f} MB, {nbytes / 1e6:.1f} MB to move -> {nbytes / med / 1e6:.0f} GB/s", flush=True)


if __name__ == "__main__":
    main()
