"""Validation of one uncropped BraTS-size case (4 x 155 x 240 x 240, windows of 128^3, overlap 16) on the calibrated
BraTS net (diagnostic, GPU): the three validation kernels alone, and evaluate.validate_seg against the per-window loop
(evaluate.sliding_window_forward + torch counts), all timed with HIP events.  Prints one JSON line.
--save-nii adds the label-map kernel (warm, and after 512 MiB of other writes have pushed the logits out of the
Infinity Cache) and validate_seg over three such cases with and without save_dir, wall time per case."""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from efficientq_amd import calibrate as K, config as Cf, evaluate as E, synth
from efficientq_amd.hip_ops import from_ndhwc, get_ops

ap = argparse.ArgumentParser()
ap.add_argument("--save-nii", dest="save_nii", action="store_true", help="also time the NIfTI label maps")
cli = ap.parse_args()
REPS = int(os.environ.get("REPS", "5"))
HBM_PEAK = 8.0e12
dev = "cuda:0"
shape, p, o = (155, 240, 240), (128, 128, 128), (16, 16, 16)


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


args = Cf.make_args(Cf.BRATS_NET, 4, 4)
QConv, _, kwQ = Cf.get_conv_class(args)
model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
synth.randomise_network(model, 0)
model.eval(); K.search_fold_and_remove_bn(model); model.to(dev); K.set_name(model)
K.calibrate_model(model, synth.calib_batch("brats", range(1), 128).to(dev), "brats", args.init_stride)
K.set_quantized(model)

g = torch.Generator().manual_seed(0)
vol = torch.randn(1, 4, *shape, generator=g).to(dev)
label = (torch.rand(3, *shape, generator=g) < 0.1).float()
ops = get_ops(dev)
nwin = 1
for n in ops.window_grid(shape, p, o):
    nwin *= n
vox, wvox = vol[0, 0].numel(), p[0] * p[1] * p[2]
win = ops.window_gather(vol, p, o)
logits_win = torch.randn(nwin, *p, 3, generator=g).to(dev)
stitched = ops.window_stitch(logits_win, (1, 3) + shape, p, o)
lab8 = label.to(dev, torch.uint8)
ops.sigmoid_threshold()
res = {"windows": nwin}
for name, fn, nbytes in (
        ("gather", lambda: ops.window_gather(vol, p, o), 4 * 4 * (vox + nwin * wvox)),
        ("stitch", lambda: ops.window_stitch(logits_win, (1, 3) + shape, p, o), 4 * 3 * (nwin * wvox + vox)),
        ("tallies", lambda: ops.seg_tallies(stitched[0], lab8, "brats"), 3 * vox * (4 + 1))):
    ms = timed(fn)
    res[name] = {"ms": round(ms, 4), "bytes": nbytes, "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}

loader = [(vol.cpu(), label[None])]


def batched():
    E.validate_seg(model, loader, "brats", p, o, window_batch=nwin)


def per_window():
    out = E.sliding_window_forward(model, loader[0][0].to(dev), p, o)[-1][0]
    pred = torch.sigmoid(out) >= 0.5
    gt = loader[0][1][0].to(dev).bool()
    torch.stack([torch.stack([(pred[c] & gt[c]).sum(), (pred[c] & ~gt[c]).sum(), (~pred[c] & gt[c]).sum(),
                              (~pred[c] & ~gt[c]).sum()]) for c in range(3)]).cpu()


res["validate_batched_ms"] = round(timed(batched, 3), 2)
res["validate_per_window_ms"] = round(timed(per_window, 3), 2)
torch.cuda.reset_peak_memory_stats()
E.validate_seg(model, loader, "brats", p, o)
res["auto_window_batch_peak_GB"] = round(torch.cuda.max_memory_allocated() / 2**30, 2)

if cli.save_nii:
    nbytes = 3 * vox * 4 + 2 * vox          # logits read, uint16 map written
    labels = lambda: ops.seg_labels(stitched, "brats", "agg", torch.uint16)
    ms = timed(labels)
    res["labels"] = {"ms": round(ms, 4), "bytes": nbytes, "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    cold = []
    for _ in range(REPS):
        evict.fill_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); labels(); b.record(); torch.cuda.synchronize()
        cold.append(a.elapsed_time(b))
    ms = sorted(cold)[len(cold) // 2]
    res["labels_after_evict"] = {"ms": round(ms, 4), "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
    del evict
    cases = loader * 3

    def wall(save_dir):
        E.validate_seg(model, cases, "brats", p, o, window_batch=nwin, fuse="agg", save_dir=save_dir,
                       multi_label="brats")
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            E.validate_seg(model, cases, "brats", p, o, window_batch=nwin, fuse="agg", save_dir=save_dir,
                           multi_label="brats")
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / len(cases))
        return round(sorted(ms)[1], 2)
    with tempfile.TemporaryDirectory() as tmp:
        res["validate_ms_per_case"] = wall(None)
        res["validate_save_nii_ms_per_case"] = wall(tmp)
        res["nii_gz_bytes"] = os.path.getsize(os.path.join(tmp, "0.nii.gz"))
print(json.dumps(res))
