"""Row f1: quantised inference over overlapped patches and the FP-vs-quantised Dice proxy.

Mirrors the reference's evaluation path for the calibrated network - ``validate_seg``'s split / per-patch
forward / stitch (``utils/validate.py:212-264``, ``utils/transforms.py:784-852``) and ``validate_vs_label``
(``utils/metrics.py:119-148``).  The per-patch forward is the calibrated ``UResQ`` in
quantized mode, i.e. every conv runs ``conv3d_quant_calib_step`` with the activation quantiser fused
(``PTQConv.py:163-167``).  ``validate_seg`` below is the HIP path of the reference's validation on labelled volumes
(batched windows, stitch, confusion counts and, with ``save_dir``, the NIfTI label maps: DESIGN.md section 13); with
``fp_model`` it also measures the calibrated network against the FP network, which needs no label.
"""
from __future__ import annotations

import math
import os
from typing import List, Sequence

import numpy as np
import torch

from .ops_window import BLEND_KINDS      # --blend: the window weights of the stitch (ops_window.blend_weights_host)


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(i) for i in v)


def window_starts(size: int, patch: int, overlap: int) -> List[int]:
    """Start offsets along one axis (transforms.py:797-800): a step of patch-overlap while a whole patch still
    ends strictly before the border, then one patch flush with the border."""
    if patch > size:
        raise RuntimeError(f"patch {patch} larger than the image extent {size}")
    if overlap >= patch:
        raise RuntimeError("overlap must be smaller than the patch")
    return list(range(0, size - patch, patch - overlap)) + [size - patch]


def image_to_patch3d(images: torch.Tensor, patch_sz, overlap) -> List[torch.Tensor]:
    """Overlapped patches of an N x C x D x H x W batch in (d, h, w) raster order (transforms.py:784-810)."""
    if patch_sz is None or overlap is None:
        return images
    p, o = _triple(patch_sz), _triple(overlap)
    d, h, w = images.shape[-3:]
    return [images[..., i:i + p[0], j:j + p[1], k:k + p[2]]
            for i in window_starts(d, p[0], o[0]) for j in window_starts(h, p[1], o[1])
            for k in window_starts(w, p[2], o[2])]


def patch_to_image3d(images: torch.Tensor, patch_list: Sequence[torch.Tensor], patch_sz, overlap) -> torch.Tensor:
    """Stitch per-patch outputs (any leading dims, e.g. heads x batch x channels) back to the image grid: sum of
    the patches over the number of patches covering each voxel (transforms.py:812-852)."""
    if patch_sz is None or overlap is None:
        return images
    p, o = _triple(patch_sz), _triple(overlap)
    d, h, w = images.shape[-3:]
    first = patch_list[0]
    acc = torch.zeros(tuple(first.shape[:-3]) + (d, h, w), dtype=first.dtype, device=first.device)
    cnt = torch.zeros((d, h, w), dtype=torch.int32, device=first.device)
    n = 0
    for i in window_starts(d, p[0], o[0]):
        for j in window_starts(h, p[1], o[1]):
            for k in window_starts(w, p[2], o[2]):
                acc[..., i:i + p[0], j:j + p[1], k:k + p[2]] += patch_list[n]
                cnt[i:i + p[0], j:j + p[1], k:k + p[2]] += 1
                n += 1
    if n != len(patch_list):
        raise RuntimeError(f"{len(patch_list)} patches for a grid of {n}")
    return acc / cnt


def dice(pred_b: torch.Tensor, target_b: torch.Tensor) -> torch.Tensor:
    """metrics.py:21-25."""
    eps = 1e-6
    return (2 * (pred_b * target_b).sum().float() + eps) / (pred_b.sum().float() + target_b.sum().float() + eps)


def validate_vs_label(output: torch.Tensor, target: torch.Tensor, task: str = "lits"):
    """Dice of the hard predictions of `output` (NCDHW logits, or M x NCDHW for M heads) against `target`
    (metrics.py:119-148): per class for lits, background + per channel for brats."""
    if output.dim() >= 6:
        return [validate_vs_label(o, target, task) for o in output]
    if task == "lits":
        pred = torch.max(output, 1)[1]
        return [dice(pred == c, target == c) for c in range(output.shape[1])]
    if task == "brats":
        pred = (torch.sigmoid(output) >= 0.5).int()
        m = [dice(pred.sum(dim=1) == 0, target.sum(dim=1) == 0)]
        return m + [dice(pred[:, c], target[:, c]) for c in range(output.shape[1])]
    raise RuntimeError(f"Unknown task {task}")


@torch.no_grad()
def sliding_window_forward(model, images: torch.Tensor, patch_size=64, overlap=16) -> torch.Tensor:
    """validate_seg's inner loop (validate.py:236-245): split, run the model on every patch, stitch.
    `model(patch)` may return one tensor or a list of heads; the result is heads x N x C x D x H x W."""
    patches = image_to_patch3d(images, patch_size, overlap)
    preds = []
    for pt in patches:
        out = model(pt.contiguous())
        if isinstance(out, (list, tuple)):
            out = torch.stack(list(out))
        elif out.dim() == images.dim():          # a single head
            out = out.unsqueeze(0)
        preds.append(out)                        # heads x N x C x d x h x w (UResQ returns its heads stacked)
    return patch_to_image3d(images, preds, patch_size, overlap)


@torch.no_grad()
def fp_vs_quantised_dice(model_q, images: torch.Tensor, task: str, fp_model=None, fp_logits=None, patch_size=64,
                         overlap=16):
    """FP-vs-Q Dice proxy (no labels offline): the hard predictions of the FP network are the target of
    the calibrated network's.  Calibration overwrites the weights in place, so the FP side must come from before
    it: either `fp_model` (a copy of the network taken before calibration, run through the same sliding window)
    or `fp_logits` (its stitched last-head logits, e.g. do_ptq's output_fp[-1]).
    Returns (dice list of the last head, stitched quantised logits, FP logits)."""
    from . import calibrate as K
    if (fp_model is None) == (fp_logits is None):
        raise ValueError("give exactly one of fp_model / fp_logits")
    if fp_logits is None:
        K.set_fp(fp_model)
        fp_logits = sliding_window_forward(fp_model, images, patch_size, overlap)[-1]
    K.set_quantized(model_q)
    out_q = sliding_window_forward(model_q, images, patch_size, overlap)[-1]
    if task == "lits":
        target = torch.max(fp_logits, 1)[1]
    else:
        target = (torch.sigmoid(fp_logits) >= 0.5).int()
    return validate_vs_label(out_q, target, task), out_q, fp_logits


# ---- validation on labelled volumes (validate.py:212-264 with metrics.py:21-45): the HIP path -----------------------
METRICS = ("dsc", "sens", "spec", "acc")
WINDOW_BATCH_MAX = 16     # windows per forward at most (a BraTS case has 8 of 128^3)
EPS = 1e-6                # metrics.py
LESION_COLUMNS = ("totall", "predl", "fnl", "fpl")     # the columns of "lesions" (hip_ops.seg_lesions)
LESION_TABLE_COLUMNS = ("d", "h", "w", "size", "overlap")   # the columns of "lesion_table" (hip_ops.seg_lesion_table)
LESION_SIZE_BINS = ((1, 9), (10, 99), (100, 999), (1000, None))    # lesion_size_summary: voxels, both ends included
SURFACE_COLUMNS = ("hd", "hd95", "assd")               # the columns of "surface" (surface_metrics), voxel units
SURFACE_COLUMNS_MM = ("hd_mm", "hd95_mm", "assd_mm")   # the same in millimetres (surface_metrics_mm)


def metrics_from_counts(counts: torch.Tensor) -> dict:
    """dice / sensitivity / specificity / accuracy per class from C x 4 counts (TP, FP, FN, TN), in the fp32
    arithmetic of metrics.py:21-45 on those same integer sums (eps included)."""
    counts = counts.to("cpu", torch.int64)
    tp, fp, fn, tn = counts.unbind(1)
    n = torch.tensor(float(counts[0].sum()), dtype=torch.float)
    return {"dsc": (2 * tp.float() + EPS) / ((tp + fp).float() + (tp + fn).float() + EPS),
            "sens": (tp.float() + EPS) / ((tp + fn).float() + EPS),
            "spec": (tn.float() + EPS) / ((tn + fp).float() + EPS),
            "acc": (tp + tn).float() / n}


def _surface_rows(rows, diag: float) -> torch.Tensor:
    """hd, hd95, assd per class (C x 3 float64) from one (n_p, n_l, max_sq, qlo_sq, qhi_sq, sum_pl, sum_lp) per class -
    the two surface counts, the largest squared distance, the two pooled order statistics squared and the two directed
    sums - and the diagonal that stands for a distance to an empty surface: the formulas of surface_metrics."""
    out = torch.zeros(len(rows), 3, dtype=torch.float64)
    for c, (n_p, n_l, max_sq, qlo, qhi, sum_pl, sum_lp) in enumerate(rows):
        if n_p == 0 and n_l == 0:
            continue
        if n_p == 0 or n_l == 0:
            out[c] = diag
            continue
        r = 95 * (n_p + n_l - 1) % 100
        lo, hi = math.sqrt(qlo), math.sqrt(qhi)
        out[c, 0] = math.sqrt(max_sq)
        out[c, 1] = lo + (hi - lo) * r / 100
        out[c, 2] = (sum_pl / n_p + sum_lp / n_l) / 2
    return out


def surface_metrics(counts, sums, shape) -> torch.Tensor:
    """hd, hd95, assd per class (C x 3 float64, voxel units) of one case of extent `shape` = (D, H, W) from what
    hip_ops.seg_surface returns: counts C x 6 = nP, nL, maxsq_PL, maxsq_LP, qlo_sq, qhi_sq and sums C x 2.  With the
    surface voxels S(P), S(L) of the predicted and the label mask and the distances of each to the other surface:
    hd = the largest of all, hd95 = the 95th percentile of the n = nP + nL pooled distances with linear interpolation
    between the order statistics (numpy.percentile: 95 (n - 1) = 100 lo + r in integers, v[lo] + (v[min(lo + 1, n - 1)]
    - v[lo]) r / 100), assd = the mean of the two directed means: medpy's hd, hd95 and assd.  Both surfaces empty: 0;
    one of them empty: sqrt(D^2 + H^2 + W^2) for all three (the BraTS convention)."""
    counts = torch.as_tensor(counts).to("cpu", torch.int64)
    sums = torch.as_tensor(sums).to("cpu", torch.float64)
    diag = math.sqrt(sum(int(e) ** 2 for e in shape))
    rows = [(n_p, n_l, max(max_pl, max_lp), qlo, qhi, *s)                   # the squares stay Python ints: sqrt is exact
            for (n_p, n_l, max_pl, max_lp, qlo, qhi), s in zip(counts.tolist(), sums.tolist())]
    return _surface_rows(rows, diag)


def surface_metrics_mm(counts, sq, sums, shape, spacing) -> torch.Tensor:
    """hd, hd95, assd per class (C x 3 float64, millimetres) of one case of extent `shape` = (D, H, W) on a grid of
    `spacing` = (d, h, w) mm from what hip_ops.seg_surface_mm returns: counts C x 2 = nP, nL, sq C x 4 fp32 = max_PL,
    max_LP, qlo, qhi (mm^2) and sums C x 2.  The definitions are surface_metrics': hd = sqrt of the larger maximum,
    hd95 = the same interpolation between sqrt(qlo) and sqrt(qhi), assd = the mean of the two directed means.  Both
    surfaces empty: 0; one of them empty: the physical diagonal sqrt(sum_a (extent_a spacing_a)^2) for all three."""
    counts = torch.as_tensor(counts).to("cpu", torch.int64)
    sq = torch.as_tensor(sq).to("cpu", torch.float64)
    sums = torch.as_tensor(sums).to("cpu", torch.float64)
    diag = math.sqrt(sum((int(e) * float(s)) ** 2 for e, s in zip(shape, spacing)))
    rows = [(*n, max(max_pl, max_lp), qlo, qhi, *s)
            for n, (max_pl, max_lp, qlo, qhi), s in zip(counts.tolist(), sq.tolist(), sums.tolist())]
    return _surface_rows(rows, diag)


def _case_geometry(geometry, i):
    """(spacing, entry) of case i: `geometry` is one spacing (d, h, w) for all cases, or one entry per case (a dict
    with `spacing` and, for the label maps, `header` / `pmin` / `pmax`: data.read_source_geometry)."""
    if isinstance(geometry, (list, tuple)) and len(geometry) == 3 and not isinstance(geometry[0], dict):
        return tuple(float(v) for v in geometry), None
    if i >= len(geometry):
        raise RuntimeError(f"validate_seg: {len(geometry)} geometries, case {i} has none")
    return tuple(float(v) for v in geometry[i]["spacing"]), geometry[i]


def _lesion_rows(rows, shape) -> np.ndarray:
    """n x 3 rows (first voxel as a linear index, size, overlap) -> n x 5 int64: d, h, w, size, overlap."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    d, h, w = np.unravel_index(r[:, 0], tuple(int(e) for e in shape))
    return np.stack([d, h, w, r[:, 1], r[:, 2]], axis=1).astype(np.int64)


def _last_head(out) -> torch.Tensor:
    """The last head of a model output: a list of heads, heads stacked in front (UResQ), or one N x C x ... tensor."""
    if isinstance(out, (list, tuple)):
        return out[-1]
    return out[-1] if out.dim() == 6 else out


def label_rule(multi: bool, multi_label=None, task: str = "lits") -> str:
    """The seg_labels rule of a validation map (validate.py:247-252 with definer.py's merge_label_func): class ids
    (argmax) without --multi_label, merge_label_brats for --multi_label brats, the merged planes (merge_label_basic)
    for --multi_label lits.  `multi_label` None with a multi-channel label: the task's own."""
    if not multi:
        return "argmax"
    key = (multi_label or task).lower()
    if key not in ("brats", "lits"):
        raise RuntimeError(f"Unknown multi_label {multi_label}")
    return "brats" if key == "brats" else "planes"


def post_class_lut(rule: str, C: int) -> list:
    """The 256-entry class table of effq_label_tallies for the maps of `rule`: bit c set = the value belongs to class c.
    argmax: class c is the value c.  brats (merge_label_brats of nested planes): WT = {1, 2, 4}, TC = {1, 4}, ET = {4}."""
    lut = [0] * 256
    if rule == "argmax":
        for c in range(C):
            lut[c] = 1 << c
    elif rule == "brats" and C == 3:
        lut[1], lut[2], lut[4] = 0b011, 0b001, 0b111
    else:
        raise RuntimeError(f"post_class_lut: no class table for the maps of rule {rule} with {C} classes")
    return lut


def post_refusal(rule: str) -> str:
    """Why the maps of `rule` cannot be cleaned and scored (validate_seg(..., post=...)), in the switches' names."""
    if rule == "planes":
        return ("--post with --multi_label lits: the prediction is one plane per class (C x D x H x W), not a label map "
                "whose components could be cleaned")
    return ("--post with --multi_label brats needs --merge_type agg or con: planes that are not nested cannot be read "
            "back from the merged label map")


def _write_map(path, host, dtype, entry=None):
    """The map of one case; with the entry of its source image (data.read_source_geometry) restored into the source's
    shape (zeros outside pmin:pmax) and written with the source's geometry."""
    from .nifti import write_nifti
    a = np.asarray(host, dtype=dtype)
    if entry is None or "header" not in entry:
        write_nifti(path, a)
        return
    if a.ndim != 3:
        raise RuntimeError(f"{path}: a map of shape {a.shape} cannot be put on the source grid (three axes needed)")
    if "pmin" in entry:
        from .data import restore_crop
        a = restore_crop(a, entry["pmin"], entry["pmax"], entry["source_shape"])
    write_nifti(path, a, geometry=entry["header"])


def _surface_entries(ops, logits, lab, kind, fuse, shape, spacing) -> dict:
    """The surface entries of one case against `lab`: "surface" and "surface_counts" in voxel units, or with a spacing
    in millimetres, then also "surface_sq" and "surface_unit"."""
    if spacing is None:
        sc, ss = ops.seg_surface(logits, lab, kind, fuse)
        sc = sc.cpu()
        return {"surface_counts": sc, "surface": surface_metrics(sc, ss, shape)}
    sc, sq, ss = ops.seg_surface_mm(logits, lab, kind, fuse, spacing)
    sc, sq = sc.cpu(), sq.cpu()
    return {"surface_counts": sc, "surface_sq": sq, "surface": surface_metrics_mm(sc, sq, ss, shape, spacing),
            "surface_unit": "mm"}


def _vs_fp(ops, q, f, kind, fuse, shape, spacing, lesions, surface, want_map) -> dict:
    """The "vs_fp" entry of one case: the calibrated network's stitched logits `q` against the FP network's `f`
    (effq_seg_agreement); for the lesion and surface entries the FP decisions are the label (seg_labels: the merged
    planes in sigmoid mode, the argmax map otherwise).  With `want_map` it also holds "map", still on the device."""
    counts, flips, stats, vmap = ops.seg_agreement(q, f, kind, fuse, want_map)
    counts, stats, S = counts.cpu(), stats.cpu(), q[0].numel()
    flips = int(flips.cpu()[0])
    out = {"counts": counts}
    out.update(metrics_from_counts(counts))
    out.update(flips=flips, flip_frac=flips / S, logit_rel_mse=stats[:, 0] / stats[:, 1], logit_max=stats[:, 2].clone(),
               prob_mae=stats[:, 3] / S)
    if lesions or surface:
        lab = ops.seg_labels(f[None], "planes" if kind == "brats" else "argmax", fuse)[0]
        if lesions:
            out["lesions"] = ops.seg_lesions(q, lab, kind, fuse).cpu()
        if surface:
            out.update(_surface_entries(ops, q, lab, kind, fuse, shape, spacing))
    if want_map:
        out["map"] = vmap
    return out


MIRROR_AXES = "dhw"                      # --tta_mirror: bit i of a flip mask mirrors axis MIRROR_AXES[i]


def mirror_flips(axes) -> tuple:
    """The flip masks of --tta_mirror `axes`, ascending: every subset of the named axes, the empty one (mask 0, the
    un-mirrored pass) included - "w" -> (0, 4), "hw" -> (0, 2, 4, 6), "dhw" -> (0, ..., 7).  None: (0,).  `axes` is a
    non-empty string over d, h, w with no letter twice; anything else is a ValueError."""
    if axes is None:
        return (0,)
    if not isinstance(axes, str) or not axes or any(a not in MIRROR_AXES for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"{axes!r}: a non-empty string over the letters d, h, w, each at most once (w, hw, dhw, ...)")
    bits = sum(1 << MIRROR_AXES.index(a) for a in axes)
    return tuple(m for m in range(8) if m & ~bits == 0)


def check_flips(flips) -> tuple:
    """`flips` as a tuple of distinct masks 0..7 in ascending order; a ValueError otherwise."""
    f = tuple(flips)
    if not f or any(isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= 7 for m in f) or \
            list(f) != sorted(set(f)):
        raise ValueError(f"flips {flips!r}: distinct flip masks 0..7 in ascending order, at least one")
    return f


@torch.no_grad()
def stitched_window_logits(ops, nets, vol: torch.Tensor, patch, overlap, window_batch=None, blend="uniform",
                           flips=(0,)):
    """The sliding-window forward of validate_seg and of the `predict` mission: the windows of `vol` (N x C x D x H x W
    fp32 on the device of `ops`) gathered into batches of `window_batch`, once per mask of `flips` and mirrored by it
    (effq_window_gather); every network of `nets` run on each; its last head un-mirrored into the network's window
    buffer, the first pass stored and the others added, so the buffer keeps its size (effq_window_put); and the buffer
    stitched and divided by the number of passes (effq_window_stitch): the logits are averaged, not the probabilities.
    window_batch=None: the first window runs alone and its peak memory - over all the forwards of `nets` - sizes the
    batches, half the free device memory at most WINDOW_BATCH_MAX windows.  Returns (one stitched N x classes x D x H x
    W tensor per network, the number of windows, the window batch in use): a caller hands the last back in for its next
    volume.
    blend: "uniform" (every covering window counts alike) or "gauss" (a window's voxels are weighted by a separable
    Gaussian of sigma = patch / 8 around its centre, hip_ops.blend_weights_host).  flips: the flip masks of mirror
    test-time augmentation (mirror_flips), ascending."""
    from .hip_ops import from_ndhwc
    if blend not in BLEND_KINDS:
        raise ValueError(f"blend {blend!r}: one of {', '.join(BLEND_KINDS)}")
    flips = check_flips(flips)
    dev = vol.device
    p, o = _triple(patch), _triple(overlap)
    bsz = window_batch
    N = int(vol.shape[0])
    nwin = 1
    for n in ops.window_grid(vol.shape[-3:], p, o):
        nwin *= n
    bufs = [None] * len(nets)
    first = 0
    while first < nwin:
        cnt = min(bsz or 1, nwin - first)
        if bsz is None:
            torch.cuda.synchronize(dev)
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
        for m in flips:                         # the peak below covers every forward of every pass
            x = from_ndhwc(ops.window_gather(vol, p, o, first, cnt, m))
            for k, net in enumerate(nets):
                last = _last_head(net(x))
                if bufs[k] is None:
                    bufs[k] = torch.empty(nwin * N, *p, int(last.shape[1]), dtype=torch.float32, device=dev)
                ops.window_put(last, bufs[k][first * N:(first + cnt) * N], m, m != flips[0])
                del last
            del x
        if bsz is None:
            per = max(1, torch.cuda.max_memory_allocated(dev) - base)
            free, _ = torch.cuda.mem_get_info(dev)
            bsz = int(max(1, min(WINDOW_BATCH_MAX, free // 2 // per)))
        first += cnt
    full = (N,) + tuple(bufs[0].shape[-1:]) + tuple(vol.shape[-3:])
    weights = None if blend == "uniform" else ops.blend_weights(p, blend)
    return [ops.window_stitch(b, full, p, o, weights, len(flips)) for b in bufs], nwin, bsz


@torch.no_grad()
def validate_seg(model, loader, task: str, patch_size, overlap, window_batch=None, fuse=None, names=None,
                 save_dir=None, label_dtype=np.uint16, multi_label=None, lesions=False, surface=False,
                 geometry=None, lesion_table=False, fp_model=None, blend="uniform", flips=(0,), post=None, post_conn=26,
                 sweep=False, lesion_match=False):
    """Validate `model` (already on its HIP device, in the mode to be measured) on every case of `loader`
    ((image N x C x D x H x W, label) batches; label = class ids N x D x H x W for lits, N x C x D x H x W 0/1 for
    brats): the case's windows gathered into batches of `window_batch` (effq_window_gather), the network run on each
    batch, the last head stitched (effq_window_stitch, bit for bit patch_to_image3d) and tallied against the label
    (effq_seg_tallies).  As in SegMetricMC.evaluate_append the label's form decides the counting, whatever `task`:
    one 0/1 channel per class (--multi_label) = sigmoid >= 0.5 per channel merged by `fuse`, class ids = argmax.
    window_batch=None: the first window runs alone and its peak memory sizes the batches, half the free device memory
    at most WINDOW_BATCH_MAX windows.  Returns one dict per case: name, counts (C x 4: TP, FP, FN, TN) and dsc / sens /
    spec / acc per class.
    save_dir: also write each case's predicted map, from the same decisions (effq_seg_labels, rule label_rule(...,
    multi_label, task)), to <save_dir>/<name>.nii.gz as `label_dtype` with the identity affine (validate.py:247-260).
    The files are written by one background thread while the device goes on; all are written when this returns.
    lesions: each dict also carries "lesions", the C x 4 int64 lesion-level counts LESION_COLUMNS of the same decisions
    (effq_seg_lesions: connected components with the 3 x 3 x 3 neighbourhood; validate_seg(..., is_cc=True),
    metrics.py:69-94) - one more call per case after the tallies.
    surface: each dict also carries "surface", the C x 3 float64 surface distances SURFACE_COLUMNS of the same decisions
    in voxel units (surface_metrics), and "surface_counts", the C x 6 int64 they come from (effq_seg_surface: an exact
    distance transform of the 2 C surfaces on the device) - one more call per case after the tallies.
    geometry: None, one spacing (d, h, w) in mm for all cases, or one entry per case (data.read_source_geometry).  The
    surface distances are then measured in millimetres (effq_seg_surface_mm, surface_metrics_mm): "surface" holds mm,
    "surface_unit" is "mm", and "surface_counts" (C x 2) and "surface_sq" (C x 4 fp32) are what they come from.  A
    case's entry with the header of its source image also puts its map on the source grid: restored into the source
    shape and written with the source's affine, codes and pixdim (a RuntimeError naming the case when the maps are the
    C x D x H x W planes of --multi_label lits, which have no place on a source grid).  Counts and metrics stay those of
    the given grid.
    lesion_table: each dict also carries "lesion_table", per class a pair (label lesions, predicted lesions) of int64
    arrays n x LESION_TABLE_COLUMNS = first voxel as d, h, w, size in voxels, overlap (the voxels the other mask of the
    class holds too; 0 = a missed / an invented lesion), in raster order of the first voxel (effq_seg_lesion_table: the
    launches of the lesion counts and four more), and with a geometry "spacing", the (d, h, w) mm of the case.  With
    lesions=True as well "lesions" comes from the same call: the case is labelled once.
    fp_model: the full-precision network (a copy taken before the calibration, on the same device, in fp mode).  Every
    batch of windows also runs through it, its last head is stitched the same way, and each dict gains "vs_fp", the
    calibrated network measured against it (effq_seg_agreement, one pass over both stitched logits): counts (C x 4 =
    both, Q only, FP only, neither - TP, FP, FN, TN with the FP decision as the truth) with dsc / sens / spec / acc,
    flips and flip_frac (voxels decided differently in any class, and their share), and per class logit_rel_mse =
    sum (q - f)^2 / sum f^2, logit_max = max |q - f| and prob_mae = mean |p_q - p_f| (p: sigmoid per channel, softmax in
    argmax mode).  With lesions / surface it also carries "lesions" / "surface" (and surface_counts, surface_sq,
    surface_unit) against the FP decisions (seg_labels of the FP logits as the label).  With save_dir the uint8 map of
    the differing classes (bit c = class c) goes to <save_dir>_vs_fp/<name>.nii.gz, on the source grid when the case has
    a source geometry.  The window batches are sized for both forwards.  A case whose label is empty (numel() == 0,
    data.SegVolumes(labels=False)) is unlabelled: it needs fp_model, takes the counting from `multi_label` (set: sigmoid
    per channel, else argmax) and its dict carries name and vs_fp only.
    blend, flips: the window weights and the mirror passes of stitched_window_logits (--blend, --tta_mirror); with
    fp_model both networks are blended and augmented alike.  Everything after the stitch is unchanged.
    post, post_conn: the rules (config.post_rules) and the neighbourhood of --post.  Each labelled case's predicted map
    (effq_seg_labels, uint8, rule label_rule(...)) is also cleaned by connected components on the given grid
    (effq_label_clean; effq_label_post when a rule fills, closes or opens) and tallied against the label
    (effq_label_tallies with post_class_lut's table), and its dict gains
    "post": counts (C x 4) with dsc / sens / spec / acc, and "changed", the voxels each rule relabelled.  Every other
    entry and the maps of save_dir stay what they are.  The planes of --multi_label lits are no label map, and the
    planes of --multi_label brats are read back from the map only when `fuse` nests them: both are a RuntimeError.
    sweep: each labelled case's dict also carries "sweep", the C x 2 x 4096 int64 histogram of the case's scores by truth
    on the host (effq_seg_sweep, one more call per case after the tallies), and "sweep_edges", the 4096 fp32 edges of its
    bins (hip_ops.sweep_edges): what sweep_summary, write_threshold_csv and write_threshold_curve_csv take.
    lesion_match: each labelled case's dict also carries "lesion_match", per class the dict of lesion_match.match_class
    (one-to-one matching of label and predicted lesions at IoU > 0.5, lesion F1, panoptic quality, lesion-wise Dice, the
    pairs of overlapping lesions) - from ops_match.seg_lesion_match (effq_seg_lesion_match), which takes the place of the
    calls of lesions / lesion_table for the case and returns their results bit for bit with the pairs."""
    from .hip_ops import get_ops
    if task not in ("lits", "brats"):
        raise RuntimeError(f"Unknown task {task}")
    post = list(post) if post else []
    dev = next(model.parameters()).device
    ops = get_ops(dev)
    p, o = _triple(patch_size), _triple(overlap)
    bsz = window_batch
    results = []
    sweep_edges = {}
    pool, writes = None, []
    if save_dir is not None:
        from concurrent.futures import ThreadPoolExecutor
        map_dtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}.get(np.dtype(label_dtype))
        if map_dtype is None:
            raise RuntimeError(f"label maps are written as uint8 or uint16, not {np.dtype(label_dtype)}")
        os.makedirs(save_dir, exist_ok=True)
        if fp_model is not None:
            os.makedirs(save_dir + "_vs_fp", exist_ok=True)
        pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="effq-nifti")
    try:
        for images, labels in loader:
            labelled = labels.numel() > 0
            if not labelled and fp_model is None:
                sn = names[len(results)] if names is not None else str(len(results))
                raise RuntimeError(f"validate_seg: case {sn} has no label: an unlabelled case is validated against the "
                                   f"FP network only (fp_model=...)")
            vol = images.to(dev, torch.float32).contiguous()
            N = int(vol.shape[0])
            nets = [model] if fp_model is None else [model, fp_model]
            outs, _, bsz = stitched_window_logits(ops, nets, vol, p, o, bsz, blend, flips)
            stitched = outs[0]
            stitched_fp = outs[1] if fp_model is not None else None
            lab = labels.to(dev).to(torch.uint8) if labelled else None
            # one 0/1 channel per class (--multi_label): sigmoid, as evaluate_append; without a label multi_label decides
            multi = lab.dim() == vol.dim() if labelled else bool(multi_label)
            kind, fz = ("brats", fuse) if multi else ("lits", None)
            maps = None
            if pool is not None:                # the planes are 0/1 uint8 on the device, cast when written
                rule = label_rule(multi, multi_label, task)
                if rule == "planes" and geometry is not None:
                    sn = names[len(results)] if names is not None else str(len(results))
                    if _case_geometry(geometry, len(results))[1] is not None:
                        raise RuntimeError(f"validate_seg: case {sn}: the maps of --multi_label lits hold one plane per "
                                           f"class (C x D x H x W); a NIfTI image has its spatial axes first, so they "
                                           f"cannot be written on the source grid: save them without --src_geom")
                maps = ops.seg_labels(stitched, rule, fuse if multi else None,
                                      torch.uint8 if rule == "planes" else map_dtype).cpu().numpy()
            post_maps = None
            if post and labelled:
                post_rule = label_rule(multi, multi_label, task)
                if post_rule == "planes" or (post_rule == "brats" and not fuse):
                    raise RuntimeError("validate_seg: post: " + post_refusal(post_rule))
                post_maps = ops.seg_labels(stitched, post_rule, fuse if multi else None, torch.uint8)
                post_lut = post_class_lut(post_rule, int(stitched.shape[1]))
            for n in range(N):
                i = len(results)
                res = {"name": names[i] if names is not None else str(i)}
                spacing, entry = _case_geometry(geometry, i) if geometry is not None else (None, None)
                if labelled:
                    counts = ops.seg_tallies(stitched[n], lab[n], kind, fz).cpu()
                    res["counts"] = counts
                    res.update(metrics_from_counts(counts))
                    if sweep:
                        res["sweep"] = ops.seg_sweep(stitched[n], lab[n], kind, fz).cpu()
                        if kind not in sweep_edges:
                            sweep_edges[kind] = ops.sweep_edges(kind)
                        res["sweep_edges"] = sweep_edges[kind]
                    if lesion_table or lesion_match:
                        if lesion_match:
                            from . import lesion_match as LM
                            from .ops_match import seg_lesion_match
                            cnt, _, rows, pairs = seg_lesion_match(ops, stitched[n], lab[n], kind, fz)
                            res["lesion_match"] = LM.case_scores(rows, pairs)
                        else:
                            cnt, _, rows = ops.seg_lesion_table(stitched[n], lab[n], kind, fz)
                        ncls = int(cnt.shape[0])
                        if lesion_table:
                            res["lesion_table"] = [(_lesion_rows(rows[ncls + c], vol.shape[-3:]),
                                                    _lesion_rows(rows[c], vol.shape[-3:])) for c in range(ncls)]
                            if spacing is not None:
                                res["spacing"] = spacing
                        if lesions:
                            res["lesions"] = cnt
                    elif lesions:
                        res["lesions"] = ops.seg_lesions(stitched[n], lab[n], kind, fz).cpu()
                    if surface:
                        res.update(_surface_entries(ops, stitched[n], lab[n], kind, fz, vol.shape[-3:], spacing))
                    if post_maps is not None:
                        cleaned, stats = ops.label_clean(post_maps[n], post, post_conn)
                        pc = ops.label_tallies(cleaned, lab[n], post_lut, int(stitched.shape[1])).cpu()
                        res["post"] = dict(metrics_from_counts(pc), counts=pc,
                                           changed=[int(v) for v in stats.cpu()[:, 1]])
                if fp_model is not None:
                    res["vs_fp"] = _vs_fp(ops, stitched[n], stitched_fp[n], kind, fz, vol.shape[-3:], spacing, lesions,
                                          surface, pool is not None)
                    if pool is not None:
                        vmap = res["vs_fp"].pop("map").cpu().numpy()
                        writes.append(pool.submit(_write_map, os.path.join(save_dir + "_vs_fp", f"{res['name']}.nii.gz"),
                                                  vmap, np.uint8, entry))
                results.append(res)
                if maps is not None and entry is None:
                    writes.append(pool.submit(_write_map, os.path.join(save_dir, f"{res['name']}.nii.gz"), maps[n],
                                              label_dtype))
                elif maps is not None:
                    writes.append(pool.submit(_write_map, os.path.join(save_dir, f"{res['name']}.nii.gz"), maps[n],
                                              label_dtype, entry))
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
    for w in writes:
        w.result()                              # re-raises a failed write
    return results


def write_metrics_csv(path: str, results) -> None:
    """One row per subject and class: subject, class, dsc, sens, spec, acc, tp, fp, fn, tn, and when the results carry
    "lesions" (validate_seg(..., lesions=True)) also totall, predl, fnl, fpl, and when they carry "surface"
    (validate_seg(..., surface=True)) after those hd, hd95, assd - named hd_mm, hd95_mm, assd_mm when the results are in
    millimetres ("surface_unit": validate_seg(..., geometry=...)); a file never mixes the two."""
    import csv
    cc = any("lesions" in r for r in results)
    sd = any("surface" in r for r in results)
    units = {r.get("surface_unit", "voxel") for r in results if "surface" in r}
    if len(units) > 1:
        raise RuntimeError("write_metrics_csv: surface distances in voxel units and in mm in one file")
    sd_cols = SURFACE_COLUMNS_MM if units == {"mm"} else SURFACE_COLUMNS
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + METRICS + ("tp", "fp", "fn", "tn") + (LESION_COLUMNS if cc else ()) +
                    (sd_cols if sd else ()))
        for r in results:
            for c in range(r["counts"].shape[0]):
                wr.writerow([r["name"], c] + ["%.7g" % float(r[m][c]) for m in METRICS] +
                            [int(v) for v in r["counts"][c]] + ([int(v) for v in r["lesions"][c]] if cc else []) +
                            (["%.7g" % float(v) for v in r["surface"][c]] if sd else []))


# ---- the threshold sweep (validate_seg(..., sweep=True), --thr_sweep) -----------------------------------------------------
SWEEP_BINS = 4096
SWEEP_MID = 2048          # the edge of the default decision: row 2048 of a sweep is the counts of metrics.csv
THRESHOLD_COLUMNS = ("subject", "class", "auc", "dsc", "best_thr_logit", "best_thr_prob", "dsc_best", "sens_best",
                     "spec_best", "pos", "neg")
THRESHOLD_CURVE_COLUMNS = ("class", "k", "thr_logit", "thr_prob", "tp", "fp", "fn", "tn", "dsc", "sens", "spec")


def _sweep_ints(hist):
    """A histogram (tensor, array or nested lists; C x 2 x 4096) as nested lists of Python integers."""
    if hasattr(hist, "tolist"):
        hist = hist.tolist()
    out = [[[int(v) for v in row] for row in cls] for cls in hist]
    if any(len(cls) != 2 or any(len(row) != SWEEP_BINS for row in cls) for cls in out):
        raise ValueError(f"a sweep histogram is C x 2 x {SWEEP_BINS}")
    return out


def sweep_pooled(hists):
    """The sum of histograms (each C x 2 x 4096) in Python integers, as nested lists."""
    hs = [_sweep_ints(h) for h in hists]
    return [[[sum(col) for col in zip(*(h[c][g] for h in hs))] for g in range(2)] for c in range(len(hs[0]))]


def sweep_summary(hist, edges):
    """Per class of a sweep histogram (C x 2 x 4096: [c][g][b] = the voxels of truth g in score bin b; hip_ops.seg_sweep, or
    sweep_pooled of several) and the 4096 edges of its bins, on the host and in integers, a dict of
      auc          (2 sum_b pos_b below_b + sum_b pos_b neg_b) / (2 P N), below_b = the negatives in the bins under b: the
                   Mann-Whitney statistic with the ties inside a bin counted half (roc_auc_score(truth, bin)); the
                   numerator is an exact Python integer; 1.0 when P = 0 or N = 0 (metrics.py:60-67)
      counts       4096 x 4 int64, row k = TP, FP, FN, TN of the decision "score >= edge k" (suffix sums; row 0: all)
      best_k       the k in 1 .. 4095 with the largest 2 TP / (2 TP + FP + FN) in fp64 (a zero denominator counts as -1);
                   ties go to the least |k - 2048|, then to the lower k
      best_thr     edge best_k as a Python float (an fp32 value)
      dsc_default, dsc_best, sens_best, spec_best    metrics_from_counts of the rows 2048 and best_k (the arithmetic of
                   metrics.csv)
      pos, neg     P and N."""
    h = _sweep_ints(hist)
    e = [float(v) for v in (edges.tolist() if hasattr(edges, "tolist") else edges)]
    if len(e) != SWEEP_BINS:
        raise ValueError(f"{len(e)} edges, a sweep has {SWEEP_BINS}")
    out = []
    for neg, pos in h:
        P, N = sum(pos), sum(neg)
        num, below = 0, 0
        for pb, nb in zip(pos, neg):
            num += 2 * pb * below + pb * nb
            below += nb
        auc = num / (2 * P * N) if P and N else 1.0
        rows, tp, fp = [None] * SWEEP_BINS, 0, 0
        for k in range(SWEEP_BINS - 1, -1, -1):
            tp += pos[k]
            fp += neg[k]
            rows[k] = (tp, fp, P - tp, N - fp)
        best_k, best = None, None
        for k in range(1, SWEEP_BINS):
            tp, fp, fn, _ = rows[k]
            den = 2 * tp + fp + fn
            key = ((2 * tp) / den if den else -1.0, -abs(k - SWEEP_MID), -k)
            if best is None or key > best:
                best_k, best = k, key
        counts = torch.tensor(rows, dtype=torch.int64)
        m = metrics_from_counts(counts[[SWEEP_MID, best_k]])
        out.append({"auc": auc, "counts": counts, "best_k": best_k, "best_thr": e[best_k],
                    "dsc_default": m["dsc"][0], "dsc_best": m["dsc"][1], "sens_best": m["sens"][1],
                    "spec_best": m["spec"][1], "pos": P, "neg": N})
    return out


def logit_prob(logit: float) -> float:
    """1 / (1 + exp(-logit)) in fp64."""
    return 1.0 / (1.0 + math.exp(-logit))


def sweep_results(results):
    """(per-subject [(name, summary)], pooled summary, edges) of the results that carry "sweep"."""
    res = [r for r in results if "sweep" in r]
    if not res:
        raise RuntimeError("no result carries a sweep (validate_seg(..., sweep=True) on labelled cases)")
    edges = res[0]["sweep_edges"]
    if any(not torch.equal(torch.as_tensor(r["sweep_edges"]), torch.as_tensor(edges)) for r in res):
        raise RuntimeError("sweeps with different edges in one file")
    per = [(r["name"], sweep_summary(r["sweep"], edges)) for r in res]
    return per, sweep_summary(sweep_pooled([r["sweep"] for r in res]), edges), edges


def write_threshold_csv(path: str, results) -> None:
    """One row per subject and class from the "sweep" entries (validate_seg(..., sweep=True)), then one row per class
    with the subject `pooled` from the summed histograms: THRESHOLD_COLUMNS.  dsc is the Dice at the default decision
    (metrics.csv's), best_thr_logit the edge of the best Dice as %.9g (the fp32 value reads back exactly),
    best_thr_prob its sigmoid in fp64."""
    import csv
    per, pooled, _ = sweep_results(results)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(THRESHOLD_COLUMNS)
        for name, summ in per + [("pooled", pooled)]:
            for c, q in enumerate(summ):
                wr.writerow([name, c, "%.9g" % q["auc"], "%.7g" % float(q["dsc_default"]), "%.9g" % q["best_thr"],
                             "%.9g" % logit_prob(q["best_thr"])] +
                            ["%.7g" % float(q[k]) for k in ("dsc_best", "sens_best", "spec_best")] + [q["pos"], q["neg"]])


def write_threshold_curve_csv(path: str, results) -> None:
    """The pooled curve of the "sweep" entries, one row per class and k = 1 .. 4095: THRESHOLD_CURVE_COLUMNS, the counts
    of the decision "score >= edge k" summed over the subjects and their dsc, sens and spec (metrics_from_counts)."""
    import csv
    _, pooled, edges = sweep_results(results)
    e = [float(v) for v in torch.as_tensor(edges).tolist()]
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(THRESHOLD_CURVE_COLUMNS)
        for c, q in enumerate(pooled):
            m = metrics_from_counts(q["counts"])
            for k in range(1, SWEEP_BINS):
                wr.writerow([c, k, "%.9g" % e[k], "%.9g" % logit_prob(e[k])] + [int(v) for v in q["counts"][k]] +
                            ["%.7g" % float(m[j][k]) for j in ("dsc", "sens", "spec")])


def write_metrics_post_csv(path: str, results) -> None:
    """One row per subject and class from the "post" entries (validate_seg(..., post=...)): subject, class, dsc, sens,
    spec, acc, tp, fp, fn, tn of the cleaned map, then changed_<k>, the voxels rule k relabelled in the subject's map
    (the same in every row of a subject)."""
    import csv
    rows = [r for r in results if "post" in r]
    nrules = max((len(r["post"]["changed"]) for r in rows), default=0)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + METRICS + ("tp", "fp", "fn", "tn") +
                    tuple(f"changed_{k}" for k in range(nrules)))
        for r in rows:
            q = r["post"]
            for c in range(q["counts"].shape[0]):
                wr.writerow([r["name"], c] + ["%.7g" % float(q[m][c]) for m in METRICS] +
                            [int(v) for v in q["counts"][c]] + [int(v) for v in q["changed"]])


def post_means(results) -> dict:
    """Per-class mean of dsc / sens / spec / acc over the "post" entries."""
    return {m: torch.stack([r["post"][m] for r in results if "post" in r]).mean(0) for m in METRICS}


AGREEMENT_COUNTS = ("both", "q_only", "fp_only", "neither")          # the columns of "vs_fp"'s counts
AGREEMENT_DRIFT = ("logit_rel_mse", "logit_max", "prob_mae")        # the per-class drift entries of "vs_fp"


def write_agreement_csv(path: str, results) -> None:
    """One row per subject and class from the "vs_fp" entries (validate_seg(..., fp_model=...)): subject, class, dsc,
    sens, spec, acc, both, q_only, fp_only, neither, flip_frac_class = (q_only + fp_only) / voxels, logit_rel_mse,
    logit_max, prob_mae, and when the entries carry "lesions" / "surface" (against the FP decisions) the columns of
    write_metrics_csv after them, under its names and its unit rule; a file never mixes voxel units and mm."""
    import csv
    vs = [(r["name"], r["vs_fp"]) for r in results if "vs_fp" in r]
    cc = any("lesions" in v for _, v in vs)
    sd = any("surface" in v for _, v in vs)
    units = {v.get("surface_unit", "voxel") for _, v in vs if "surface" in v}
    if len(units) > 1:
        raise RuntimeError("write_agreement_csv: surface distances in voxel units and in mm in one file")
    sd_cols = SURFACE_COLUMNS_MM if units == {"mm"} else SURFACE_COLUMNS
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class") + METRICS + AGREEMENT_COUNTS + ("flip_frac_class",) + AGREEMENT_DRIFT +
                    (LESION_COLUMNS if cc else ()) + (sd_cols if sd else ()))
        for name, v in vs:
            for c in range(v["counts"].shape[0]):
                row = [int(n) for n in v["counts"][c]]
                wr.writerow([name, c] + ["%.7g" % float(v[m][c]) for m in METRICS] + row +
                            ["%.7g" % ((row[1] + row[2]) / sum(row))] +
                            ["%.7g" % float(v[k][c]) for k in AGREEMENT_DRIFT] +
                            ([int(n) for n in v["lesions"][c]] if cc else []) +
                            (["%.7g" % float(n) for n in v["surface"][c]] if sd else []))


def agreement_means(results) -> dict:
    """Means over the cases of the "vs_fp" entries: dsc, logit_rel_mse and prob_mae per class, and flip_frac."""
    vs = [r["vs_fp"] for r in results if "vs_fp" in r]
    out = {k: torch.stack([v[k].to(torch.float64) for v in vs]).mean(0) for k in ("dsc", "logit_rel_mse", "prob_mae")}
    out["flip_frac"] = sum(v["flip_frac"] for v in vs) / len(vs)
    return out


def write_lesions_csv(path: str, results) -> None:
    """One row per lesion of results that carry "lesion_table" (validate_seg(..., lesion_table=True)): subject, class,
    kind (label | pred), lesion (1-based, in raster order of the first voxel: scipy.ndimage.label's number), d, h, w of
    the first voxel, size in voxels, overlap; per subject and class the label lesions first.  When the results carry a
    "spacing" a last column vol_mm3 = size x voxel volume; a file never mixes rows with and without it.  When they carry
    "lesion_match" (validate_seg(..., lesion_match=True)) three more columns after all others: match (the 1-based number
    of the lesion of the other kind matched one to one at IoU > 0.5, or 0), best_iou (the largest IoU with any lesion of
    the other kind, or 0) and partners (how many of them it shares voxels with); again a file never mixes the two."""
    import csv
    res = [r for r in results if "lesion_table" in r]
    mm = {"spacing" in r for r in res}
    if len(mm) > 1:
        raise RuntimeError("write_lesions_csv: cases with and without a spacing in one file")
    mm = mm == {True}
    lm = {"lesion_match" in r for r in res}
    if len(lm) > 1:
        raise RuntimeError("write_lesions_csv: cases with and without a lesion matching in one file")
    lm = lm == {True}
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(("subject", "class", "kind", "lesion") + LESION_TABLE_COLUMNS + (("vol_mm3",) if mm else ()) +
                    (("match", "best_iou", "partners") if lm else ()))
        for r in res:
            vox = float(np.prod([float(v) for v in r["spacing"]])) if mm else None
            for c, pair in enumerate(r["lesion_table"]):
                for kind, rows in zip(("label", "pred"), pair):
                    side = r["lesion_match"][c][kind] if lm else None
                    for k, row in enumerate(np.asarray(rows, dtype=np.int64).reshape(-1, 5)):
                        wr.writerow([r["name"], c, kind, k + 1] + [int(v) for v in row] +
                                    (["%.7g" % (int(row[3]) * vox)] if mm else []) +
                                    ([int(side["match"][k]), "%.7g" % float(side["best_iou"][k]),
                                      int(side["partners"][k])] if lm else []))


def lesion_size_summary(results) -> np.ndarray:
    """The label lesions of results that carry "lesion_table" per class and size bin (LESION_SIZE_BINS: 1-9, 10-99,
    100-999, >= 1000 voxels): C x 4 x 2 int64 = the lesions of the bin over all cases, and how many of them were
    detected (overlap > 0)."""
    res = [r for r in results if "lesion_table" in r]
    out = np.zeros((max((len(r["lesion_table"]) for r in res), default=0), len(LESION_SIZE_BINS), 2), np.int64)
    for r in res:
        for c, (label_rows, _) in enumerate(r["lesion_table"]):
            rows = np.asarray(label_rows, dtype=np.int64).reshape(-1, 5)
            for b, (lo, hi) in enumerate(LESION_SIZE_BINS):
                sel = (rows[:, 3] >= lo) & ((rows[:, 3] <= hi) if hi is not None else True)
                out[c, b, 0] += int(sel.sum())
                out[c, b, 1] += int((sel & (rows[:, 4] > 0)).sum())
    return out


def metric_means(results) -> dict:
    """Per-class mean over the cases of each metric."""
    return {m: torch.stack([r[m] for r in results]).mean(0) for m in METRICS}


def lesion_totals(results) -> torch.Tensor:
    """Per-class sums over the cases of the lesion-level counts (C x 4 int64: LESION_COLUMNS)."""
    return torch.stack([r["lesions"].to("cpu", torch.int64) for r in results]).sum(0)


def surface_means(results) -> torch.Tensor:
    """Per-class means over the cases of the surface distances (C x 3 float64: SURFACE_COLUMNS)."""
    return torch.stack([r["surface"].to("cpu", torch.float64) for r in results]).mean(0)
