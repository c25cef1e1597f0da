"""Row f1: quantised inference over overlapped patches and the FP-vs-quantised Dice proxy.

Mirrors the reference's evaluation path for the calibrated network - ``validate_seg``'s split / per-patch
forward / stitch (``utils/validate.py:212-264``, ``utils/transforms.py:784-852``) and ``validate_vs_label``
(``utils/metrics.py:119-148``).  The per-patch forward is the calibrated ``UResQ`` in
quantized mode, i.e. every conv runs ``conv3d_quant_calib_step`` with the activation quantiser fused
(``PTQConv.py:163-167``).  ``validate_seg`` below is the HIP path of the reference's validation on labelled volumes
(batched windows, stitch, confusion counts and, with ``save_dir``, the NIfTI label maps: DESIGN.md section 13); with
``fp_model`` it also measures the calibrated network against the FP network, which needs no label.

This module keeps the validation loop and what a case's entries are made of.  The sliding window lives in window.py,
the host arithmetic over counts and results in metrics.py, the CSV writers and the printed reports in reports.py; every
name of theirs is imported here, so ``evaluate.X`` is what it always was.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np
import torch

from .metrics import (AGREEMENT_COUNTS, AGREEMENT_DRIFT, EPS, LESION_COLUMNS, LESION_SIZE_BINS,      # noqa: F401
                      LESION_TABLE_COLUMNS, METRICS, SURFACE_COLUMNS, SURFACE_COLUMNS_MM, SWEEP_BINS, SWEEP_MID,
                      _surface_rows, _sweep_ints, agreement_means, dice, lesion_size_summary, lesion_totals, logit_prob,
                      metric_means, metrics_from_counts, post_means, surface_means, surface_metrics, surface_metrics_mm,
                      sweep_pooled, sweep_results, sweep_summary, validate_vs_label)
from .nifti import BackgroundWriter, write_nifti
from .reports import (THRESHOLD_COLUMNS, THRESHOLD_CURVE_COLUMNS, write_agreement_csv, write_lesions_csv,      # noqa: F401
                      write_metrics_csv, write_metrics_post_csv, write_threshold_csv, write_threshold_curve_csv)
from .window import (BLEND_KINDS, MIRROR_AXES, WINDOW_BATCH_MAX, _last_head, _triple, check_flips,      # noqa: F401
                     image_to_patch3d, mirror_flips, patch_to_image3d, sliding_window_forward, stitched_window_logits,
                     window_starts)


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


# ---- validation on labelled volumes (validate.py:212-264 with metrics.py:21-45): the HIP path -----------------------
# the optional entries of a labelled case: validate_seg's switches of the same names
_Want = namedtuple("_Want", "lesions surface lesion_table lesion_match sweep post post_conn")
# what a loader batch decides for every case in it: kind, the counting ("brats" = sigmoid >= 0.5 per channel, "lits" =
# argmax); fuse, the merge in force (validate_seg's `fuse` with one channel per class, else None); rule, label_rule of the
# maps (None when neither save_dir nor post needs a map)
_Batch = namedtuple("_Batch", "labelled kind fuse rule")


def _case_name(names, i) -> str:
    return names[i] if names is not None else str(i)


def _batch_decisions(images, labels, i, names, task, fuse, multi_label, with_fp, save, post, geometry) -> _Batch:
    """The _Batch of (images, labels), whose first case is case `i`, or the RuntimeError of what it cannot do.
    As in SegMetricMC.evaluate_append the label's form decides the counting, whatever `task`: one 0/1 channel per class
    (--multi_label) = sigmoid >= 0.5 per channel merged by `fuse`, class ids = argmax.  A batch whose label is empty
    (numel() == 0, data.SegVolumes(labels=False)) is unlabelled: it needs the FP network and takes the counting from
    `multi_label` (set: sigmoid per channel, else argmax).  Maps on a source grid (save_dir with a per-case geometry)
    cannot be the C x D x H x W planes of --multi_label lits; post needs a label map: the planes of --multi_label lits
    are none, and the planes of --multi_label brats are read back from the map only when `fuse` nests them."""
    labelled = labels.numel() > 0
    if not labelled and not with_fp:
        raise RuntimeError(f"validate_seg: case {_case_name(names, i)} has no label: an unlabelled case is validated "
                           f"against the FP network only (fp_model=...)")
    multi = labels.dim() == images.dim() if labelled else bool(multi_label)
    rule = label_rule(multi, multi_label, task) if save or (post and labelled) else None
    if save and rule == "planes" and geometry is not None and _case_geometry(geometry, i)[1] is not None:
        raise RuntimeError(f"validate_seg: case {_case_name(names, i)}: the maps of --multi_label lits hold one plane per "
                           f"class (C x D x H x W); a NIfTI image has its spatial axes first, so they "
                           f"cannot be written on the source grid: save them without --src_geom")
    if post and labelled and (rule == "planes" or (rule == "brats" and not fuse)):
        raise RuntimeError("validate_seg: post: " + post_refusal(rule))
    return _Batch(labelled, "brats" if multi else "lits", fuse if multi else None, rule)


def _labelled_entries(ops, logits, lab, b: _Batch, want: _Want, shape, spacing, post_map, post_lut, edges) -> dict:
    """The entries of one labelled case (stitched logits C x D x H x W against its label), in the order of the device
    calls - tallies, sweep, lesion table or match or lesions, surface, post:
    counts (C x 4: TP, FP, FN, TN, effq_seg_tallies) and dsc / sens / spec / acc per class.
    sweep: "sweep", the C x 2 x 4096 int64 histogram of the case's scores by truth on the host (effq_seg_sweep, one more
    call per case after the tallies), and "sweep_edges", the 4096 fp32 edges of its bins (hip_ops.sweep_edges, kept in
    `edges` per kind): what sweep_summary, write_threshold_csv and write_threshold_curve_csv take.
    lesions: "lesions", the C x 4 int64 lesion-level counts LESION_COLUMNS of the same decisions (effq_seg_lesions:
    connected components with the 3 x 3 x 3 neighbourhood; validate_seg(..., is_cc=True), metrics.py:69-94) - one more
    call per case after the tallies.
    lesion_table: "lesion_table", per class a pair (label lesions, predicted lesions) of int64 arrays n x
    LESION_TABLE_COLUMNS = first voxel as d, h, w, size in voxels, overlap (the voxels the other mask of the class holds
    too; 0 = a missed / an invented lesion), in raster order of the first voxel (effq_seg_lesion_table: the launches of
    the lesion counts and four more), and with a geometry "spacing", the (d, h, w) mm of the case.  With lesions as well
    "lesions" comes from the same call: the case is labelled once.
    lesion_match: "lesion_match", per class the dict of lesion_match.match_class (one-to-one matching of label and
    predicted lesions at IoU > 0.5, lesion F1, panoptic quality, lesion-wise Dice, the pairs of overlapping lesions) -
    from ops_match.seg_lesion_match (effq_seg_lesion_match), which takes the place of the calls of lesions /
    lesion_table for the case and returns their results bit for bit with the pairs.
    surface: "surface", the C x 3 float64 surface distances SURFACE_COLUMNS of the same decisions in voxel units
    (surface_metrics), and "surface_counts", the C x 6 int64 they come from (effq_seg_surface: an exact distance
    transform of the 2 C surfaces on the device) - one more call per case after the tallies.  With a `spacing` they are
    measured in millimetres (effq_seg_surface_mm, surface_metrics_mm): "surface" holds mm, "surface_unit" is "mm", and
    "surface_counts" (C x 2) and "surface_sq" (C x 4 fp32) are what they come from.
    post (with `post_map`, the case's uint8 map of rule b.rule, and `post_lut`, post_class_lut's table): the map cleaned
    by connected components on the given grid (effq_label_clean; effq_label_post when a rule fills, closes or opens) and
    tallied against the label (effq_label_tallies): "post" = counts (C x 4) with dsc / sens / spec / acc, and "changed",
    the voxels each rule relabelled.  Every other entry and the maps of save_dir stay what they are."""
    counts = ops.seg_tallies(logits, lab, b.kind, b.fuse).cpu()
    res = {"counts": counts}
    res.update(metrics_from_counts(counts))
    if want.sweep:
        res["sweep"] = ops.seg_sweep(logits, lab, b.kind, b.fuse).cpu()
        if b.kind not in edges:
            edges[b.kind] = ops.sweep_edges(b.kind)
        res["sweep_edges"] = edges[b.kind]
    if want.lesion_table or want.lesion_match:
        if want.lesion_match:
            from . import lesion_match as LM
            from .ops_match import seg_lesion_match
            cnt, _, rows, pairs = seg_lesion_match(ops, logits, lab, b.kind, b.fuse)
            res["lesion_match"] = LM.case_scores(rows, pairs)
        else:
            cnt, _, rows = ops.seg_lesion_table(logits, lab, b.kind, b.fuse)
        ncls = int(cnt.shape[0])
        if want.lesion_table:
            res["lesion_table"] = [(_lesion_rows(rows[ncls + c], shape), _lesion_rows(rows[c], shape))
                                   for c in range(ncls)]
            if spacing is not None:
                res["spacing"] = spacing
        if want.lesions:
            res["lesions"] = cnt
    elif want.lesions:
        res["lesions"] = ops.seg_lesions(logits, lab, b.kind, b.fuse).cpu()
    if want.surface:
        res.update(_surface_entries(ops, logits, lab, b.kind, b.fuse, shape, spacing))
    if post_map is not None:
        cleaned, stats = ops.label_clean(post_map, want.post, want.post_conn)
        pc = ops.label_tallies(cleaned, lab, post_lut, int(logits.shape[0])).cpu()
        res["post"] = dict(metrics_from_counts(pc), counts=pc, changed=[int(v) for v in stats.cpu()[:, 1]])
    return res


@torch.no_grad()
def validate_seg(model, loader, task: str, patch_size, overlap, window_batch=None, fuse=None, names=None,
                 save_dir=None, label_dtype=np.uint16, multi_label=None, lesions=False, surface=False,
                 geometry=None, lesion_table=False, fp_model=None, blend="uniform", flips=(0,), post=None, post_conn=26,
                 sweep=False, lesion_match=False):
    """Validate `model` (already on its HIP device, in the mode to be measured) on every case of `loader`
    ((image N x C x D x H x W, label) batches; label = class ids N x D x H x W for lits, N x C x D x H x W 0/1 for
    brats): the case's windows gathered into batches of `window_batch` (effq_window_gather), the network run on each
    batch, the last head stitched (effq_window_stitch, bit for bit patch_to_image3d) and tallied against the label
    (effq_seg_tallies); the label's form decides the counting (_batch_decisions).
    window_batch=None: the first window runs alone and its peak memory sizes the batches, half the free device memory
    at most WINDOW_BATCH_MAX windows.  Returns one dict per case: name, then the entries of a labelled case
    (_labelled_entries: counts and dsc / sens / spec / acc per class, and what lesions, surface, lesion_table, post,
    post_conn (the rules of config.post_rules and the neighbourhood of --post), sweep and lesion_match add), then vs_fp.
    save_dir: also write each case's predicted map, from the same decisions (effq_seg_labels, rule label_rule(...,
    multi_label, task)), to <save_dir>/<name>.nii.gz as `label_dtype` with the identity affine (validate.py:247-260).
    The files are written by one background thread while the device goes on; all are written when this returns.
    geometry: None, one spacing (d, h, w) in mm for all cases, or one entry per case (data.read_source_geometry).  The
    surface distances are then measured in millimetres.  A case's entry with the header of its source image also puts
    its map on the source grid: restored into the source shape and written with the source's affine, codes and pixdim
    (a RuntimeError naming the case when the maps are the C x D x H x W planes of --multi_label lits, which have no
    place on a source grid).  Counts and metrics stay those of the given grid.
    fp_model: the full-precision network (a copy taken before the calibration, on the same device, in fp mode).  Every
    batch of windows also runs through it, its last head is stitched the same way, and each dict gains "vs_fp", the
    calibrated network measured against it (effq_seg_agreement, one pass over both stitched logits): counts (C x 4 =
    both, Q only, FP only, neither - TP, FP, FN, TN with the FP decision as the truth) with dsc / sens / spec / acc,
    flips and flip_frac (voxels decided differently in any class, and their share), and per class logit_rel_mse =
    sum (q - f)^2 / sum f^2, logit_max = max |q - f| and prob_mae = mean |p_q - p_f| (p: sigmoid per channel, softmax in
    argmax mode).  With lesions / surface it also carries "lesions" / "surface" (and surface_counts, surface_sq,
    surface_unit) against the FP decisions (seg_labels of the FP logits as the label).  With save_dir the uint8 map of
    the differing classes (bit c = class c) goes to <save_dir>_vs_fp/<name>.nii.gz, on the source grid when the case has
    a source geometry.  The window batches are sized for both forwards.  The dict of an unlabelled case carries name
    and vs_fp only.
    blend, flips: the window weights and the mirror passes of stitched_window_logits (--blend, --tta_mirror); with
    fp_model both networks are blended and augmented alike.  Everything after the stitch is unchanged."""
    from . import hip_ops
    if task not in ("lits", "brats"):
        raise RuntimeError(f"Unknown task {task}")
    want = _Want(lesions, surface, lesion_table, lesion_match, sweep, list(post) if post else [], post_conn)
    dev = next(model.parameters()).device
    ops = hip_ops.get_ops(dev)
    p, o = _triple(patch_size), _triple(overlap)
    nets = [model] if fp_model is None else [model, fp_model]
    bsz = window_batch
    results, sweep_edges = [], {}
    save = save_dir is not None
    if save:
        map_dtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}.get(np.dtype(label_dtype))
        if map_dtype is None:
            raise RuntimeError(f"label maps are written as uint8 or uint16, not {np.dtype(label_dtype)}")
        os.makedirs(save_dir, exist_ok=True)
        if fp_model is not None:
            os.makedirs(save_dir + "_vs_fp", exist_ok=True)
    with BackgroundWriter("effq-nifti") as writer:
        for images, labels in loader:
            b = _batch_decisions(images, labels, len(results), names, task, fuse, multi_label, fp_model is not None,
                                 save, want.post, geometry)
            vol = images.to(dev, torch.float32).contiguous()
            outs, _, bsz = stitched_window_logits(ops, nets, vol, p, o, bsz, blend, flips)
            stitched = outs[0]
            lab = labels.to(dev).to(torch.uint8) if b.labelled else None
            shape = vol.shape[-3:]
            maps = post_maps = post_lut = None
            if save:                            # the planes are 0/1 uint8 on the device, cast when written
                maps = ops.seg_labels(stitched, b.rule, b.fuse,
                                      torch.uint8 if b.rule == "planes" else map_dtype).cpu().numpy()
            if want.post and b.labelled:
                post_maps = ops.seg_labels(stitched, b.rule, b.fuse, torch.uint8)
                post_lut = post_class_lut(b.rule, int(stitched.shape[1]))
            for n in range(int(vol.shape[0])):
                i = len(results)
                res = {"name": _case_name(names, i)}
                spacing, entry = _case_geometry(geometry, i) if geometry is not None else (None, None)
                if b.labelled:
                    res.update(_labelled_entries(ops, stitched[n], lab[n], b, want, shape, spacing,
                                                 post_maps[n] if post_maps is not None else None, post_lut, sweep_edges))
                if fp_model is not None:
                    res["vs_fp"] = _vs_fp(ops, stitched[n], outs[1][n], b.kind, b.fuse, shape, spacing, lesions, surface,
                                          save)
                    if save:
                        vmap = res["vs_fp"].pop("map").cpu().numpy()
                        writer.submit(_write_map, os.path.join(save_dir + "_vs_fp", f"{res['name']}.nii.gz"), vmap,
                                      np.uint8, entry)
                results.append(res)
                if save:
                    writer.submit(_write_map, os.path.join(save_dir, f"{res['name']}.nii.gz"), maps[n], label_dtype,
                                  entry)
    return results
