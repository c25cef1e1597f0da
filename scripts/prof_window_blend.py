"""Time the window kernels of the sliding window on the device: the cases of DESIGN section 16.

    python scripts/prof_window_blend.py [--launches 20]

Per case (a BraTS-sized and a LiTS-sized volume, three channels in and out): random values of 4 N(0, 1) on the device,
one warm-up launch, then `--launches` launches, each between a pair of device events; the median, the least and the
greatest are printed, and for a row that sits beside another the ratio of the medians: window_stitch with weights to
window_stitch without, window_gather(flip = 7) to window_gather(flip = 0), window_put to the copy_(permute) that stored
the last head before it.  The last two rows are one whole evaluate.stitched_window_logits call with its defaults on the
BraTS-sized volume, every window in one batch, through a toy network (half its input): once with the head as a
contiguous N x C x pd x ph x pw tensor, what the put and the copy_(permute) rows take, and once with the channels-last
strides of its input, what the project's own convs return (window_put first makes such a head contiguous)."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd.evaluate import stitched_window_logits  # noqa: E402
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
        rows = [("stitch, weights None", None, lambda: ops.window_stitch(win, full, p, o)),
                ("stitch, ones", "stitch, weights None", lambda: ops.window_stitch(win, full, p, o, ones, 1)),
                ("stitch, gauss, nflip 8", "stitch, weights None", lambda: ops.window_stitch(win, full, p, o, gauss, 8)),
                ("gather, flip 0", None, lambda: ops.window_gather(vol, p, o, 0, cnt, 0)),
                ("gather, flip 7", "gather, flip 0", lambda: ops.window_gather(vol, p, o, 0, cnt, 7)),
                ("copy_(permute)", None, lambda: dst.copy_(last.permute(0, 2, 3, 4, 1))),
                ("put, flip 0, store", "copy_(permute)", lambda: ops.window_put(last, dst, 0, False)),
                ("put, flip 7, store", "copy_(permute)", lambda: ops.window_put(last, dst, 7, False)),
                ("put, flip 7, add", "copy_(permute)", lambda: ops.window_put(last, dst, 7, True))]
        if name == "brats-sized":
            for head, net in (("NCDHW", lambda x: (0.5 * x).contiguous()), ("channels-last", lambda x: 0.5 * x)):
                rows.append((f"stitched_window_logits, defaults, toy network, {head} head", None,
                             lambda net=net: stitched_window_logits(ops, [net], vol, p, o, window_batch=nwin)))
        print(f"{name}: volume {shape}, C = {C}, windows {p} overlap {o}: {nwin} windows, {cnt} per gather / put",
              flush=True)
        med = {}
        for what, beside, fn in rows:
            med[what], lo, hi = timed(fn, a.launches)
            ratio = f", {med[what] / med[beside]:.2f} x {beside}" if beside else ""
            print(f"  {what}: median {med[what]:.3f} ms (min {lo:.3f}, max {hi:.3f}) of {a.launches}{ratio}", flush=True)


if __name__ == "__main__":
    main()
