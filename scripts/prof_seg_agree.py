"""Validation against the FP network on one uncropped BraTS-size case (3 x 155 x 240 x 240 logits; diagnostic, GPU),
timed with HIP events, one JSON line per step.
--step kernel: effq_seg_agreement alone (both modes, with and without the map, warm and after 512 MiB of other writes
  have pushed the logits out of the Infinity Cache) next to the existing calls that give its counts, seg_labels of the FP
  logits + seg_tallies against that map (three launches).  hbm_frac = the bytes the call must move (the 2 x 3 planes of
  logits, the map when written; for the three calls the 2 x 3 planes, the label planes written and read) over the time
  and the 8 TB/s peak.
--step validate: evaluate.validate_seg per case on the calibrated BraTS net (windows of 128^3, overlap 16) with and
  without fp_model, alternating, wall time with a device synchronise."""
import argparse, copy, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from efficientq_amd import calibrate as K, config as Cf, evaluate as E, synth
from efficientq_amd.hip_ops import get_ops

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=["kernel", "validate"], required=True)
cli = ap.parse_args()
REPS = int(os.environ.get("REPS", "7"))
HBM_PEAK = 8.0e12
dev = "cuda:0"
shape, p, o = (155, 240, 240), (128, 128, 128), (16, 16, 16)
vox = shape[0] * shape[1] * shape[2]
ops = get_ops(dev)
g = torch.Generator().manual_seed(0)


def timed(fn, reps=REPS, before=None):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


if cli.step == "kernel":
    f = torch.randn(3, *shape, generator=g).to(dev)
    q = (f + 0.3 * torch.randn(3, *shape, generator=g).to(dev)).contiguous()
    ops.sigmoid_threshold()
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    res = {"voxels": vox}
    logit_bytes = 2 * 3 * vox * 4

    def three_calls(mode, fuse):
        if mode == "argmax":
            return ops.seg_tallies(q, ops.seg_labels(f[None], "argmax")[0], "lits")
        return ops.seg_tallies(q, ops.seg_labels(f[None], "planes", fuse)[0], "brats", fuse)

    for mode, fuse, lab_bytes in (("argmax", None, 2 * vox), ("sigmoid", "agg", 2 * 3 * vox)):
        for name, fn, nbytes in (
                (f"agreement_{mode}", lambda: ops.seg_agreement(q, f, mode, fuse), logit_bytes),
                (f"agreement_{mode}_map", lambda: ops.seg_agreement(q, f, mode, fuse, want_map=True), logit_bytes + vox),
                (f"labels_tallies_{mode}", lambda: three_calls(mode, fuse), logit_bytes + lab_bytes)):
            ms, cold = timed(fn), timed(fn, before=lambda: evict.fill_(1))
            res[name] = {"ms": round(ms, 4), "ms_after_evict": round(cold, 4), "bytes": nbytes,
                         "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                         "hbm_frac_after_evict": round(nbytes / (cold * 1e-3) / HBM_PEAK, 3)}
        same = torch.equal(ops.seg_agreement(q, f, mode, fuse)[0], three_calls(mode, fuse))
        res[f"counts_equal_{mode}"] = bool(same)
    print(json.dumps(res))
else:
    args = Cf.make_args(Cf.BRATS_NET, 4, 4)
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(model, 0)
    model.eval(); K.search_fold_and_remove_bn(model); model.to(dev); K.set_name(model)
    fp = copy.deepcopy(model)
    K.set_fp(fp)
    K.calibrate_model(model, synth.calib_batch("brats", range(1), 128).to(dev), "brats", args.init_stride)
    K.set_quantized(model)
    vol = torch.randn(1, 4, *shape, generator=g)
    label = (torch.rand(1, 3, *shape, generator=g) < 0.1).float()
    loader = [(vol, label)]

    def wall(**kw):
        torch.cuda.synchronize()
        t0 = time.time()
        r = E.validate_seg(model, loader, "brats", p, o, fuse="agg", multi_label="brats", **kw)
        torch.cuda.synchronize()
        return time.time() - t0, r

    wall(); wall(fp_model=fp)
    plain, both = [], []
    for _ in range(3):
        plain.append(wall()[0])
        t, r = wall(fp_model=fp)
        both.append(t)
    vs = r[0]["vs_fp"]
    print(json.dumps({"validate_s": round(sorted(plain)[1], 3), "validate_vs_fp_s": round(sorted(both)[1], 3),
                      "dsc": [round(float(v), 4) for v in vs["dsc"]], "flip_frac": round(vs["flip_frac"], 5),
                      "logit_rel_mse": [float("%.4g" % float(v)) for v in vs["logit_rel_mse"]],
                      "prob_mae": [float("%.4g" % float(v)) for v in vs["prob_mae"]]}))
