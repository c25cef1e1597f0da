"""effq_seg_sweep beside effq_seg_tallies on the logits of one uncropped BraTS-size case (3 x 155 x 240 x 240), on the
same buffers (diagnostic, GPU): the median of REPS (5) HIP-event pairs after a warm-up call, as scripts/time_validation.py
times the table of DESIGN.md section 13.  Prints one JSON line.

Cases: sigmoid mode with a background-heavy volume (97 % of the voxels far below -16, an empty label there), without a
merge and with `agg`; argmax mode with C = 3 on the same logits; and two synthetic extremes that bracket the histogram's
cost - every voxel in one bin (one LDS add per wave and key) and Gaussian logits of sigma 4 (up to 64 distinct bins per
wave: the ballot rounds and then one LDS add per lane)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from efficientq_amd.hip_ops import get_ops

REPS = int(os.environ.get("REPS", "5"))
HBM_PEAK = 8.0e12
dev = "cuda:0"
shape = (155, 240, 240)
C = 3


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


ops = get_ops(dev)
ops.sigmoid_threshold()
g = torch.Generator().manual_seed(0)
vox = shape[0] * shape[1] * shape[2]
fg = torch.rand(shape, generator=g) < 0.03
noise = torch.randn(C, *shape, generator=g)
heavy = torch.where(fg[None], 3.0 * noise, -30.0 + noise).to(dev)                 # background: far below the first edge
lab_planes = (fg[None] & (torch.rand(C, *shape, generator=g) < 0.5)).to(dev, torch.uint8)
lab_ids = (fg.long() * torch.randint(0, C, shape, generator=g)).to(dev, torch.uint8)
one_bin = torch.full((C,) + shape, -3.3, device=dev)
gauss = (4.0 * noise).to(dev)
res = {"voxels": vox, "classes": C, "reps": REPS}
for key, logits, lab, task, fuse in (("sigmoid_background_heavy", heavy, lab_planes, "brats", None),
                                     ("sigmoid_agg_background_heavy", heavy, lab_planes, "brats", "agg"),
                                     ("argmax_background_heavy", heavy, lab_ids, "lits", None),
                                     ("sigmoid_one_bin", one_bin, lab_planes, "brats", None),
                                     ("sigmoid_gauss4", gauss, lab_planes, "brats", None),
                                     ("argmax_gauss4", gauss, lab_ids, "lits", None)):
    sweep = timed(lambda: ops.seg_sweep(logits, lab, task, fuse))
    tallies = timed(lambda: ops.seg_tallies(logits, lab, task, fuse))
    hist = ops.seg_sweep(logits, lab, task, fuse)
    counts = ops.seg_tallies(logits, lab, task, fuse)
    row = torch.stack([hist[:, 1, 2048:].sum(1), hist[:, 0, 2048:].sum(1), hist[:, 1, :2048].sum(1),
                       hist[:, 0, :2048].sum(1)], 1)
    nbytes = vox * (4 * C + (C if task == "brats" else 1))
    res[key] = {"sweep_ms": round(sweep, 4), "tallies_ms": round(tallies, 4), "ratio": round(sweep / tallies, 2),
                "bytes": nbytes, "sweep_hbm_frac": round(nbytes / (sweep * 1e-3) / HBM_PEAK, 3),
                "tallies_hbm_frac": round(nbytes / (tallies * 1e-3) / HBM_PEAK, 3),
                "plan": ops.seg_sweep_plan(C, vox, task), "row_2048_is_tallies": bool(torch.equal(row, counts)),
                "bins_in_use": int((hist.sum(1) > 0).sum())}
print(json.dumps(res))
