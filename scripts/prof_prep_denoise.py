"""Times of the non-local means filter on one 240 x 240 x 155 volume: effq_prep_denoise_nlm at nlm1,
nlm3 and nlm5 and the residual pass, one warm-up and then --repeat launches between device events each; median with min
and max, and the rate in voxel-candidate pairs per second over the voxels of the mask.

    python scripts/prof_prep_denoise.py [--repeat 20]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd import denoise as N, ops_denoise as O      # noqa: E402
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
    ap.add_argument("--repeat", type=int, default=20)
    repeat = ap.parse_args().repeat
    ops = get_ops("cuda:0")
    shape = (240, 240, 155)
    z = np.stack(np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")).astype(np.float32)
    g = np.random.default_rng(0)
    body = (z ** 2).sum(0) < 1.2                      # a head-sized ball in a background of zeros
    v = np.where(body, 500 + 300 * (z[0] > 0) + 200 * (z[1] * z[2] > 0.1) + 20 * g.standard_normal(shape), 0)
    v = torch.from_numpy(v.astype(np.float32)).to("cuda:0")
    inside = int(body.sum())
    sigma, n = N.noise_sigma(ops, "timing", "t1", v)
    print(f"{shape}: {inside} of {body.size} voxels in the mask, sigma {sigma:.2f} from {n} residuals")
    print("residual %.3f ms (%.3f - %.3f)" % times_ms(lambda: O.prep_denoise_residual(ops, v), repeat))
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    y, change = torch.empty_like(v), torch.empty(2, dtype=torch.float64, device="cuda:0")
    for mask, voxels in (("nonzero", inside), ("all", body.size)):
        for radius in (1, 3, 5):
            def launch():                             # the launches alone: no read-back between the events
                rc = ops.lib.effq_prep_denoise_nlm(v.data_ptr(), *shape, {"nonzero": 0, "all": 1}[mask], radius,
                                                   sigma * sigma, y.data_ptr(), change.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), ops.stream)
                assert rc == 0, rc
            med, lo, hi = times_ms(launch, repeat)
            pairs = voxels * ((2 * radius + 1) ** 3 - 1)
            sumsq, count = change.cpu().tolist()
            print(f"nlm{radius} mask {mask}: {med:.3f} ms ({lo:.3f} - {hi:.3f}), {pairs / med / 1e6:.1f} G pairs / s, "
                  f"rms removed {np.sqrt(sumsq / count):.2f} over {int(count)} voxels")


if __name__ == "__main__":
    main()
