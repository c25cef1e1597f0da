"""Time the window kernels of the blend and of mirror test-time augmentation on the device: the cases of DESIGN section 16.

    python scripts/prof_window_blend.py [--launches 20]

Per case (a BraTS-sized and a LiTS-sized volume, three channels in and out): random values of 4 N(0, 1) on the device,
one warm-up launch, then `--launches` launches, each between a pair of device events; the median, the least and the
greatest are printed, and for every new kernel the ratio of its median to the median of the kernel it sits beside:
window_stitch_weighted to window_stitch, window_gather_flip(flip = 7) to window_gather, window_put to the
copy_(permute) it replaces."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd.hip_ops import get_ops  # noqa: E402

# name, channels, volume (D, H, W), window, overlap
CASES = [("brats-sized", 3, (240, 240, 155), (128, 128, 128), (16, 16, 16)),
         ("lits-sized", 3, (512, 512, 200), (128, 128, 64), (16, 16, 16))]


def timed(fn, launches):
    fn()                                                                        # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(torch.cuda.current_stream())
        fn()
        t1.record(torch.cuda.current_stream())
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8, help="windows per gather / put, as one forward takes them")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = get_ops(dev)
    for name, C, shape, p, o in CASES:
        nwin = math.prod(ops.window_grid(shape, p, o))
        cnt = min(a.batch, nwin)
        vol = 4.0 * torch.randn((1, C) + shape, device=dev)
        win = 4.0 * torch.randn((nwin,) + p + (C,), device=dev)
        last = 4.0 * torch.randn((cnt, C) + p, device=dev)
        ones, gauss = ops.blend_weights(p, "uniform"), ops.blend_weights(p, "gauss")
        full = (1, C) + shape
        dst = win[:cnt]
        rows = [("window_stitch", None, lambda: ops.window_stitch(win, full, p, o)),
                ("window_stitch_weighted, ones", "window_stitch",
                 lambda: ops.window_stitch_weighted(win, full, p, o, ones, 1)),
                ("window_stitch_weighted, gauss, nflip 8", "window_stitch",
                 lambda: ops.window_stitch_weighted(win, full, p, o, gauss, 8)),
                ("window_gather", None, lambda: ops.window_gather(vol, p, o, 0, cnt)),
                ("window_gather_flip, flip 0", "window_gather", lambda: ops.window_gather_flip(vol, p, o, 0, cnt, 0)),
                ("window_gather_flip, flip 7", "window_gather", lambda: ops.window_gather_flip(vol, p, o, 0, cnt, 7)),
                ("copy_(permute)", None, lambda: dst.copy_(last.permute(0, 2, 3, 4, 1))),
                ("window_put, flip 0, store", "copy_(permute)", lambda: ops.window_put(last, dst, 0, False)),
                ("window_put, flip 7, store", "copy_(permute)", lambda: ops.window_put(last, dst, 7, False)),
                ("window_put, flip 7, add", "copy_(permute)", lambda: ops.window_put(last, dst, 7, True))]
        print(f"{name}: volume {shape}, C = {C}, windows {p} overlap {o}: {nwin} windows, {cnt} per gather / put",
              flush=True)
        med = {}
        for what, beside, fn in rows:
            med[what], lo, hi = timed(fn, a.launches)
            ratio = f", {med[what] / med[beside]:.2f} x {beside}" if beside else ""
            print(f"  {what}: median {med[what]:.3f} ms (min {lo:.3f}, max {hi:.3f}) of {a.launches}{ratio}", flush=True)


if __name__ == "__main__":
    main()
