"""Times of the bias field correction on one 240 x 240 x 155 volume: one fit iteration (the histogram
call, the host sharpening and the fit call, and the fit call's three kernels alone) at stride 4 and at stride 1, the apply
pass, and one whole correction (wall clock, repeated after a warm-up run).  Medians over --repeat runs after a warm-up, device time from events around the calls.

    python scripts/time_prep_bias.py [--repeat 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd import bias as B, ops_bias as O          # noqa: E402
from efficientq_amd.hip_ops import get_ops                    # noqa: E402


def median_ms(fn, repeat):
    for _ in range(3):
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
    ap.add_argument("--repeat", type=int, default=20)
    repeat = ap.parse_args().repeat
    ops = get_ops("cuda:0")
    shape = (240, 240, 155)
    z = np.stack(np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")).astype(np.float32)
    g = np.random.default_rng(0)
    body = (z ** 2).sum(0) < 1.2
    v = np.where(body, (500 + 300 * (z[0] > 0) + 20 * g.standard_normal(shape)) * np.exp(0.2 * z[1] * z[2] + 0.1 * z[0]), 0)
    v = torch.from_numpy(v.astype(np.float32)).to("cuda:0")
    u, m = O.prep_bias_log(ops, v)
    for stride, offset in (((4, 4, 4), (2, 2, 2)), ((1, 1, 1), (0, 0, 0))):
        f = torch.zeros(O.sample_shape(shape, stride, offset), dtype=torch.float32, device="cuda:0")
        counters, lo, hi, n = O.prep_bias_hist(ops, u, m, f, stride, offset)
        table = B.sharpen(counters / 65536.0, lo, hi)
        for level in (0, 3):
            cells = (2 ** level + 3) ** 3
            phi, lat = (torch.zeros(cells, dtype=torch.float64, device="cuda:0") for _ in range(2))

            def whole():
                c, a, b, _ = O.prep_bias_hist(ops, u, m, f, stride, offset)
                O.prep_bias_fit(ops, u, m, f, stride, offset, level, a, b, B.sharpen(c / 65536.0, a, b), phi, lat)

            def fit_only():
                O.prep_bias_fit(ops, u, m, f, stride, offset, level, lo, hi, table, phi, lat)
            print(f"stride {stride[0]} level {level} ({n} samples): iteration %.3f ms (%.3f - %.3f), fit call %.3f ms "
                  f"(%.3f - %.3f)" % (median_ms(whole, repeat) + median_ms(fit_only, repeat)))
    lattices = torch.from_numpy(0.05 * g.standard_normal(O.LATTICE)).to("cuda:0")
    print("apply %.3f ms (%.3f - %.3f)" % median_ms(lambda: O.prep_bias_apply(ops, v, m, lattices), repeat))
    walls = []
    for _ in range(1 + max(repeat // 4, 3)):                 # the first run is the warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        _, done = B.correct(ops, "timing", "t1", v)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t)
    print(f"whole correction {statistics.median(walls[1:]):.4f} s of wall clock ({min(walls[1:]):.4f} - {max(walls[1:]):.4f}, "
          f"{len(walls) - 1} runs; the first {walls[0]:.4f}), iterations {done.iters}, field {done.field_min:.3f} - "
          f"{done.field_max:.3f}")


if __name__ == "__main__":
    main()
