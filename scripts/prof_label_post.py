"""Time whole calls of effq_label_post (HipOps.label_clean with fill / closeR / openR rules) on the device: the cost table
of DESIGN section 21.

    python scripts/prof_label_post.py [--calls 400] [--windows 5]

A 155 x 240 x 240 map (the size of section 17's table) made from a seed: an ellipsoid body of label 1 with a lesion of
label 2 inside it, pin-holes of label 0 at density 0.002 inside both, and specks of both labels at density 0.001 each
around them.  Per chain of rules: five warm-up calls, then `--windows` windows of `--calls` calls between a pair of
device events; the median, the least and the greatest time per call are printed with the rule's counters.  For context
the same chain is then run once on the host through the numpy / scipy restatement of tests/label_morph_ref.py, timed by
the host clock, and compared with the device's map and counters."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd.hip_ops import get_ops  # noqa: E402
from tests import label_morph_ref as M  # noqa: E402

CHAINS = {
    "1,2:fill>1": [((1, 2), "fill", 0, 1)],
    "1,2:close3>1": [((1, 2), "close", 3, 1)],
    "2:open1>1": [((2,), "open", 1, 1)],
    "the three in a chain": [((1, 2), "fill", 0, 1), ((1, 2), "close", 3, 1), ((2,), "open", 1, 1)],
    "1,2:largest (effq_label_clean)": [((1, 2), "largest", 0, 0)],
}


def make_map(D=155, H=240, W=240, seed=0):
    g = np.random.default_rng(seed)
    z, y, x = np.ogrid[:D, :H, :W]
    body = ((z - 77) / 50.0) ** 2 + ((y - 120) / 80.0) ** 2 + ((x - 120) / 70.0) ** 2 <= 1.0
    lesion = ((z - 80) / 12.0) ** 2 + ((y - 100) / 15.0) ** 2 + ((x - 130) / 15.0) ** 2 <= 1.0
    a = np.zeros((D, H, W), dtype=np.uint8)
    a[body] = 1
    a[lesion] = 2
    r = g.random((D, H, W))
    a[body & (r < 0.002)] = 0
    a[~body & (r < 0.001)] = 1
    a[~body & (r > 0.999)] = 2
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    ops = get_ops(dev)
    a = make_map()
    print("map", a.shape, "voxels per label", np.bincount(a.ravel()).tolist(), flush=True)
    m = torch.from_numpy(a).to(dev)
    for name, rules in CHAINS.items():
        for _ in range(5):
            out, stats = ops.label_clean(m, rules, 26)
        torch.cuda.synchronize()
        per = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                out, stats = ops.label_clean(m, rules, 26)
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) / args.calls)
        per.sort()
        print(f"{name}: median {per[len(per) // 2]:.3f} ms, least {per[0]:.3f}, greatest {per[-1]:.3f}, "
              f"stats {stats.cpu().tolist()}", flush=True)
        t = time.perf_counter()
        want, wstats = M.post(a, rules, 26)
        host = time.perf_counter() - t
        same = np.array_equal(out.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), wstats)
        print(f"   host restatement {host:.2f} s, equal to the device: {same}", flush=True)
    D, H, W = a.shape
    print("workspace at radius 3 and without a ball:", ops.lib.effq_label_post_ws_bytes(D, H, W, 3),
          ops.lib.effq_label_post_ws_bytes(D, H, W, 0))


if __name__ == "__main__":
    main()
