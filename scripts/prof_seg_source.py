"""Time effq_seg_labels_source (HipOps.seg_labels_source) on the device: the cases of DESIGN section 15.

    python scripts/prof_seg_source.py [--launches 20]

Source grids are (SD, SH, SW) as the kernel takes them: a scan's array axes i, j, k, so SW - the axis a row item takes
four voxels of - is the last one.  Per case: random logits of 4 N(0, 1) on the device, one warm-up launch, then
`--launches` launches, each between a pair of device events; the median, the least and the greatest are printed beside
the bytes the pass must move (the logits once, the labels once)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd.hip_ops import get_ops  # noqa: E402

# name, source (SD, SH, SW), factors, box (pmin, extent) or None for the whole grid, rule, fuse
CASES = [("lits-sized, f = 1, whole grid", (512, 512, 200), None, None, "argmax", None),
         ("lits-sized, f = (1, 1, 2.5), whole grid", (512, 512, 200), (1.0, 1.0, 2.5), None, "argmax", None),
         ("lits-sized, slices first, f = 1, whole grid", (200, 512, 512), None, None, "argmax", None),
         ("brats-sized, f = 1, whole grid", (240, 240, 155), None, None, "brats", "con"),
         ("brats-sized, f = 1, box", (240, 240, 155), None, ((50, 40, 10), (140, 160, 128)), "brats", "con"),
         ("brats-sized, slices first, f = 1, whole grid", (155, 240, 240), None, None, "brats", "con")]


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
        out = ops.seg_labels_source(logits, pmin, G, f, src, rule, fuse)      # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(a.launches):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(torch.cuda.current_stream())
            out = ops.seg_labels_source(logits, pmin, G, f, src, rule, fuse)
            t1.record(torch.cuda.current_stream())
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        nbytes = logits.numel() * 4 + out.numel()
        med = statistics.median(times)
        print(f"{name}: source (SD, SH, SW) = {src}, grid {tuple(G)}, box {tuple(ext)} at {tuple(pmin)}, C = {a.classes}, "
              f"{rule}/{fuse}: median {med:.3f} ms (min {min(times):.3f}, max {max(times):.3f}) of {a.launches}; "
              f"{nbytes / 1e6:.1f} MB to move -> {nbytes / med / 1e6:.0f} GB/s", flush=True)


if __name__ == "__main__":
    main()
