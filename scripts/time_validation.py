"""Validation of one uncropped BraTS-size case (4 x 155 x 240 x 240, windows of 128^3, overlap 16) on the calibrated
BraTS net (diagnostic, GPU): the three validation kernels alone, and evaluate.validate_seg against the per-window loop
(evaluate.sliding_window_forward + torch counts), all timed with HIP events.  Prints one JSON line.
--save-nii adds the label-map kernel (warm, and after 512 MiB of other writes have pushed the logits out of the
Infinity Cache) and validate_seg over three such cases with and without save_dir, wall time per case.
--is-cc adds effq_seg_lesions (the lesion-level columns: connected components of the 2 x 3 masks of the case) on the
calibrated net's own stitched logits and on random logits (masks of density 0.5: one giant component with holes), with
validate_seg per case with and without lesions=True, and - where scipy is importable - the reference's way on the same
masks (device -> host copy + ndimage.label of the label mask and the predicted mask of each class).  The time per phase
is read from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python scripts/time_validation.py --is-cc).
--surf-dist adds effq_seg_surface (the surface distances hd, hd95, assd: an exact distance transform of the 2 x 3
surfaces of the case) in the same way: on the net's own logits and on random logits, validate_seg per case with and
without surface=True, and with scipy the host way on the same masks (copy + two binary erosions and two
distance_transform_edt per class).
--surf-dist --spacing d,h,w times effq_seg_surface_mm (the same distances in millimetres on a grid of that spacing: the
weighted transform and the radix select) the same way, next to the integer path measured in the same run, and
validate_seg per case with geometry=spacing.
--lesion-table adds effq_seg_lesion_table (one record per lesion: the launches of --is-cc and four more) on the net's own
logits and on random logits, called as the library is (a table of 2^18 rows per plane, no host read), next to
effq_seg_lesions in the same run, validate_seg per case with lesion_table=True, and with scipy the host way on the same
masks (copy + ndimage.label + numpy.bincount of both masks of each class).  The time per phase is read from a kernel
trace (rocprofv3 --kernel-trace --stats -- python scripts/time_validation.py --lesion-table)."""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from efficientq_amd import calibrate as K, config as Cf, evaluate as E, synth
from efficientq_amd.hip_ops import from_ndhwc, get_ops

ap = argparse.ArgumentParser()
ap.add_argument("--save-nii", dest="save_nii", action="store_true", help="also time the NIfTI label maps")
ap.add_argument("--is-cc", dest="is_cc", action="store_true", help="also time the lesion-level counts")
ap.add_argument("--surf-dist", dest="surf_dist", action="store_true", help="also time the surface distances")
ap.add_argument("--lesion-table", dest="lesion_table", action="store_true", help="also time the per-lesion table")
ap.add_argument("--spacing", default=None, help="d,h,w in mm: with --surf-dist also time the distances in mm")
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

if cli.is_cc:
    # the calibrated net's own logits of the case, stitched as validate_seg stitches them
    with torch.no_grad():
        out = E._last_head(model(from_ndhwc(win)))
    net_logits = ops.window_stitch(out.permute(0, 2, 3, 4, 1).contiguous(), (1, 3) + shape, p, o)
    planes = 6
    # algorithmic bytes: logits and label read, 2 B of decision bits written and read by the tiles and the flatten, 4 B
    # labels written by the tiles, read by the merge's surface voxels (about half), read and written by the flatten,
    # read by the count; 1 B flags zeroed and read
    nbytes = vox * (3 * 5 + 2 * 3) + planes * vox * (4 * 4.5 + 2)
    for key, lg in (("lesions", net_logits), ("lesions_random_logits", stitched)):
        ms = timed(lambda: ops.seg_lesions(lg[0], lab8, "brats", "agg"))
        res[key] = {"ms": round(ms, 4), "bytes": int(nbytes), "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                    "counts": ops.seg_lesions(lg[0], lab8, "brats", "agg").tolist()}
    res["cc_ws_MB"] = round(ops.lib.effq_cc_ws_bytes(planes, *shape) / 1e6, 1)

    def wall_cc(lesions):
        ms = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.validate_seg(model, loader * 3, "brats", p, o, window_batch=nwin, fuse="agg", lesions=lesions)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / 3)
        return round(sorted(ms[1:])[1], 2)
    res["validate_ms_per_case"] = wall_cc(False)
    res["validate_lesions_ms_per_case"] = wall_cc(True)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    res["scipy"] = ndimage is not None
    if ndimage is not None:
        import numpy as np
        pred = ops.seg_labels(net_logits, "planes", "agg")[0]

        def host_way():
            pm, gm = pred.cpu().numpy(), lab8.cpu().numpy()
            return [ndimage.label(m[c], np.ones((3, 3, 3)))[1] for c in range(3) for m in (gm, pm)]
        host_way()
        ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_way()
            ms.append((time.perf_counter() - t0) * 1e3)
        res["scipy_label_ms"] = round(sorted(ms)[1], 1)
        res["scipy_over_kernel"] = round(res["scipy_label_ms"] / res["lesions"]["ms"], 1)
if cli.lesion_table:
    import ctypes as C
    from efficientq_amd import _lib
    with torch.no_grad():
        out = E._last_head(model(from_ndhwc(win)))
    net_logits = ops.window_stitch(out.permute(0, 2, 3, 4, 1).contiguous(), (1, 3) + shape, p, o)
    planes, cap = 6, 1 << 18
    counts = torch.empty(3, 4, dtype=torch.int64, device=dev)
    nrows = torch.empty(planes, dtype=torch.int64, device=dev)
    rows = torch.empty(planes, cap, 3, dtype=torch.int32, device=dev)
    need = ops.lib.effq_cc_table_ws_bytes(planes, *shape, cap)
    ws = ops._workspace("cc", need)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    thresh = ops.sigmoid_threshold()

    def table(lg):
        _lib.check(ops.lib.effq_seg_lesion_table(ptr(lg), ptr(lab8), 3, *shape, _lib.SEG_SIGMOID, _lib.SEG_FUSE["agg"],
                                                 thresh, _lib.LESION_CONNECTIVITY, cap, ptr(counts), ptr(nrows), ptr(rows),
                                                 ptr(ws), ws.numel(), ops.stream), "effq_seg_lesion_table")
    for key, lg in (("lesion_table", net_logits[0].contiguous()), ("lesion_table_random_logits", stitched[0].contiguous())):
        ms = timed(lambda: table(lg))
        ms_cc = timed(lambda: ops.seg_lesions(lg, lab8, "brats", "agg"))
        n = nrows.tolist()
        sizes = [rows[q, :min(n[q], cap), 1] for q in range(planes)]
        res[key] = {"ms": round(ms, 4), "lesions_ms": round(ms_cc, 4), "nrows": n,
                    "largest": [int(s.max()) if s.numel() else 0 for s in sizes],
                    "counts_equal": bool(torch.equal(counts, ops.seg_lesions(lg, lab8, "brats", "agg")))}
    res["cc_table_ws_MB"] = round(need / 1e6, 1)
    res["cc_ws_MB"] = round(ops.lib.effq_cc_ws_bytes(planes, *shape) / 1e6, 1)

    def wall_table(**kw):
        ms = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.validate_seg(model, loader * 3, "brats", p, o, window_batch=nwin, fuse="agg", **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / 3)
        return round(sorted(ms[1:])[1], 2)
    res["validate_ms_per_case"] = wall_table()
    res["validate_lesions_ms_per_case"] = wall_table(lesions=True)
    res["validate_lesion_table_ms_per_case"] = wall_table(lesions=True, lesion_table=True)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    res["scipy"] = ndimage is not None
    if ndimage is not None:
        import numpy as np
        pred = ops.seg_labels(net_logits, "planes", "agg")[0]

        def host_way():
            pm, gm = pred.cpu().numpy(), lab8.cpu().numpy()
            out = []
            for c in range(3):
                for m, other in ((gm[c], pm[c]), (pm[c], gm[c])):
                    lab, n = ndimage.label(m, np.ones((3, 3, 3)))
                    out.append((np.bincount(lab.reshape(-1), minlength=n + 1)[1:],
                                np.bincount(lab.reshape(-1)[other.reshape(-1) != 0], minlength=n + 1)[1:]))
            return out
        ms = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_way()
            ms.append((time.perf_counter() - t0) * 1e3)
        res["scipy_table_ms"] = round(min(ms), 1)
        res["scipy_over_kernel"] = round(res["scipy_table_ms"] / res["lesion_table"]["ms"], 1)
if cli.surf_dist:
    with torch.no_grad():
        out = E._last_head(model(from_ndhwc(win)))
    net_logits = ops.window_stitch(out.permute(0, 2, 3, 4, 1).contiguous(), (1, 3) + shape, p, o)
    planes = 6
    # algorithmic bytes: logits and label read, 2 B of decision bits written and read, 2 B of surface bits written and
    # read by the rows (once per plane) and the histogram; 4 B of squared distance per plane written by the rows, read
    # and written by each of the two line passes; the histogram's reads of the maps are left out (surface voxels only)
    nbytes = vox * (3 * 5 + 2 * 2 + 2 * 2) + planes * vox * (2 + 4 * 5)
    for key, lg in (("surface", net_logits), ("surface_random_logits", stitched)):
        ms = timed(lambda: ops.seg_surface(lg[0], lab8, "brats", "agg"))
        cnt, sm = ops.seg_surface(lg[0], lab8, "brats", "agg")
        res[key] = {"ms": round(ms, 4), "bytes": int(nbytes), "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                    "counts": cnt.tolist(), "metrics": E.surface_metrics(cnt, sm, shape).tolist()}
    res["surf_ws_MB"] = round(ops.lib.effq_surf_ws_bytes(planes, *shape) / 1e6, 1)

    def wall_sd(surface):
        ms = []
        for i in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.validate_seg(model, loader * 3, "brats", p, o, window_batch=nwin, fuse="agg", surface=surface)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / 3)
        return round(sorted(ms[1:])[2], 2)
    res["validate_ms_per_case"] = wall_sd(False)
    res["validate_surface_ms_per_case"] = wall_sd(True)
    if cli.spacing:
        spacing = tuple(float(v) for v in cli.spacing.split(","))
        # the same traffic as the integer path (fp32 maps for int32 ones); the select reads the surface bits four more
        # times (2 B per voxel each) and the maps at the surface voxels only
        nbytes_mm = nbytes + 4 * vox * 2
        for key, lg in (("surface_mm", net_logits), ("surface_mm_random_logits", stitched)):
            ms = timed(lambda: ops.seg_surface_mm(lg[0], lab8, "brats", "agg", spacing))
            cnt, sq, sm = ops.seg_surface_mm(lg[0], lab8, "brats", "agg", spacing)
            res[key] = {"ms": round(ms, 4), "bytes": int(nbytes_mm),
                        "hbm_frac": round(nbytes_mm / (ms * 1e-3) / HBM_PEAK, 3), "counts": cnt.tolist(),
                        "metrics_mm": E.surface_metrics_mm(cnt, sq, sm, shape, spacing).tolist()}
            res[key]["over_integer_path"] = round(ms / res[key.replace("_mm", "")]["ms"], 2)
        res["surf_mm_ws_MB"] = round(ops.lib.effq_surf_mm_ws_bytes(planes, *shape) / 1e6, 1)

        def wall_mm():
            ms = []
            for i in range(6):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                E.validate_seg(model, loader * 3, "brats", p, o, window_batch=nwin, fuse="agg", surface=True,
                               geometry=spacing)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / 3)
            return round(sorted(ms[1:])[2], 2)
        res["validate_surface_mm_ms_per_case"] = wall_mm()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    res["scipy"] = ndimage is not None
    if ndimage is not None and not cli.spacing:
        import numpy as np
        pred = ops.seg_labels(net_logits, "planes", "agg")[0]
        six = ndimage.generate_binary_structure(3, 1)

        def host_way():
            pm, gm = pred.cpu().numpy() != 0, lab8.cpu().numpy() != 0
            out = []
            for c in range(3):
                sp, sl = pm[c] & ~ndimage.binary_erosion(pm[c], six), gm[c] & ~ndimage.binary_erosion(gm[c], six)
                if not sp.any() or not sl.any():
                    out.append(None)
                    continue
                dpl, dlp = ndimage.distance_transform_edt(~sl)[sp], ndimage.distance_transform_edt(~sp)[sl]
                pooled = np.hstack([dpl, dlp])
                out.append((pooled.max(), np.percentile(pooled, 95), (dpl.mean() + dlp.mean()) / 2))
            return out
        ms = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = host_way()
            ms.append((time.perf_counter() - t0) * 1e3)
        res["scipy_surface_ms"] = round(min(ms), 1)
        res["scipy_metrics"] = [None if h is None else [float(v) for v in h] for h in host]
        res["scipy_over_kernel"] = round(res["scipy_surface_ms"] / res["surface"]["ms"], 1)
print(json.dumps(res))
