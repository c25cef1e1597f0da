"""Time whole calls of effq_label_lesions and effq_label_surface_mm on the device: the figures of DESIGN section 26.

    python scripts/time_label_score.py [--reps 7] [--calls 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/time_label_score.py --reps 1 --calls 5

One BraTS-size case, 155 x 240 x 240 at spacing (5, 0.7421875, 0.7421875) mm, made from a seed: smoothed noise thresholded
into nested labels 2, 1, 4 (whole tumour, core, enhancing), the prediction the truth shifted by (1, 2, 3) voxels; scored with the
BraTS classes.  Per entry: three warm-up calls, then `--reps` windows of `--calls` calls between a pair of device events;
the median, the least and the greatest time per call.  For context the entry points that take logits run on one-hot
logits of the same maps (three argmax classes are not the nested ones: a context figure, not a comparison of equals)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientq_amd import config as Cf  # noqa: E402
from efficientq_amd.hip_ops import get_ops  # noqa: E402
from efficientq_amd.ops_score import label_lesions, label_surface_mm  # noqa: E402

SHAPE = (155, 240, 240)
SPACING = (5.0, 0.7421875, 0.7421875)
TOLS8 = (0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 13.0, 21.0)


def make_maps(seed=0):
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn((1, 1) + tuple(n // 4 + 2 for n in SHAPE), generator=g)
    smooth = torch.nn.functional.interpolate(noise, scale_factor=4, mode="trilinear", align_corners=False)[0, 0]
    smooth = smooth[:SHAPE[0] + 4, :SHAPE[1] + 4, :SHAPE[2] + 4]

    def labels(f):
        a = torch.zeros(f.shape, dtype=torch.uint8)
        a[f > 0.6] = 2
        a[f > 0.9] = 1
        a[f > 1.2] = 4
        return a
    truth = labels(smooth[:SHAPE[0], :SHAPE[1], :SHAPE[2]])
    pred = labels(smooth[1:SHAPE[0] + 1, 2:SHAPE[1] + 2, 3:SHAPE[2] + 3])
    return pred.contiguous(), truth.contiguous()


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
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    ops = get_ops(dev)
    pred, truth = (t.to(dev) for t in make_maps())
    classes = Cf.SCORE_CLASSES["brats"]
    lut = Cf.score_class_lut(classes)
    counts, _, _, within = label_surface_mm(ops, pred, truth, lut, 3, SPACING, TOLS8)
    print("voxels per label, pred", torch.bincount(pred.reshape(-1)).tolist(), "truth",
          torch.bincount(truth.reshape(-1)).tolist())
    print("surface voxels (nP, nL) per class", counts.tolist(), "within at 21 mm", within[:, :, -1].tolist(), flush=True)
    ids = torch.tensor([0, 1, 2, 0, 3], dtype=torch.long, device=dev)          # label value -> argmax class 0..3
    x = torch.nn.functional.one_hot(ids[pred.long()], 4).permute(3, 0, 1, 2).float().contiguous()
    lab = ids[truth.long()].to(torch.uint8)
    entries = [
        ("label_surface_mm, no tolerance", lambda: label_surface_mm(ops, pred, truth, lut, 3, SPACING)),
        ("label_surface_mm, 1 tolerance", lambda: label_surface_mm(ops, pred, truth, lut, 3, SPACING, (1.0,))),
        ("label_surface_mm, 8 tolerances", lambda: label_surface_mm(ops, pred, truth, lut, 3, SPACING, TOLS8)),
        ("label_lesions", lambda: label_lesions(ops, pred, truth, lut, 3)),
        ("label_tallies", lambda: ops.label_tallies(pred, truth, lut, 3)),
        ("seg_surface_mm on one-hot logits, 4 argmax classes", lambda: ops.seg_surface_mm(x, lab, "lits", None, SPACING)),
        ("seg_lesions on one-hot logits, 4 argmax classes", lambda: ops.seg_lesions(x, lab, "lits")),
    ]
    for rnd in range(2):                    # twice: the spread between rounds is the noise of the figures
        for name, fn in entries:
            med, lo, hi = timed(fn, args.reps, args.calls)
            print(f"round {rnd}: {name}: median {med:.3f} ms, least {lo:.3f}, greatest {hi:.3f}", flush=True)


if __name__ == "__main__":
    main()
