"""The ``predict`` mission: segment new scans with a calibrated snapshot and write label maps that overlay the scans.

    python -m efficientq_amd.entrance predict --config config/lits_ptq.yaml --qlvl_w 4 --qlvl_a 4 \
        --resume out/state_in_fp.pkl --src_list new_cases.csv --out_dir seg/ \
        [--prep_window -200,250 --prep_spacing 1,1,2.5 --prep_mask all --prep_min_size d,h,w --patch_size d,h,w]
        [--prep_align MODALITY] [--prep_orient RAS] [--prep_antialias] [--prep_interp cubic]
        [--blend gauss --tta_mirror hw]

``--src_list`` is the CSV of the ``prep`` mission (prep.read_src_list; a ``seg`` column is allowed and ignored).  The
``--prep_*`` switches and ``--patch_size`` mean what they mean in ``prep`` and ``ptq`` and have the same per-task
defaults (``--prep_min_size``: the patch); they must be what the calibration data was prepared with, and the values used
are written into ``predict.csv``.  The network is exactly one of ``--resume`` (a snapshot of the ``ptq`` mission,
calibrate.load_calibrated) and ``--pretrain`` with ``--qconv conv`` (the FP checkpoint, folded as do_ptq folds it).

Per subject: the scans are read (the next subject's by one background thread, prep.read_subjects), windowed, resampled,
standardised and cropped in memory (prep.process_subject under prep.PrepOptions, the option set prep shares), the windows
of the crop run through the network and the last head is stitched (window.stitched_window_logits), and effq_seg_labels_source turns the stitched logits on the working grid into one
label per voxel of the scan's own grid: ``<out_dir>/<subject>.nii.gz``, uint8, with the header of the first modality
(of the reference under ``--prep_align``),
written by a background thread (nifti.BackgroundWriter).  ``<out_dir>/predict.csv`` gets one row per subject: the source shape and spacing, the
grid, the box, the number of windows, the prep options used, and per label value present in the map its voxel count
(counted on the device) and its volume in ml.

``--prep_orient CODE`` reorients the working arrays as ``prep`` does (it must be what the calibration data was prepared
with): effq_seg_labels_source then writes the map on the oriented source grid, and one effq_prep_reorient of that uint8
map with the inverse plan puts it on the scan's own grid before ``--post``, the counts, the copy and the write, so the file
still has the scan's header and overlays it.  ``predict.csv`` then gains the columns ``source_orient`` (the scan's own
code) and ``orient`` after those of the list above and before the blend and post columns.

``--prep_antialias`` (with ``--prep_spacing``) filters the images before they are down-sampled as ``prep`` does (pass
what the calibration data was prepared with).  ``predict.csv`` then gains the column ``antialias`` (the sigmas of the
three array axes, ``0 0 0`` for a subject with nothing to filter) after the orient columns and before those of
``--blend``; without ``--prep_spacing`` the switch is refused by name.

``--prep_interp cubic`` (with ``--prep_spacing``) resamples the images by cubic B-spline interpolation as ``prep`` does
(pass what the calibration data was prepared with).  ``predict.csv`` then gains the column ``interp`` (``cubic``) after
the ``antialias`` column's place and before those of ``--blend``; the step back to the scan's grid stays trilinear on
the logits.  ``linear``, the default, changes nothing; another value, or cubic without ``--prep_spacing``, is refused by
name.

``--prep_align MODALITY`` names the reference modality as in ``prep``: every other modality whose header lies on another
grid is resampled onto the reference's grid by the affines as they stand (effq_prep_align; no registration), before
everything else.  The map is written on the reference's grid with the reference's header.  ``predict.csv`` then gains
the columns ``align`` and ``align_inside`` (per modality the voxels of the grid inside that scan's field of view) after
the ``interp`` column's place and before ``window_bounds`` and those of ``--blend``.

``--prep_window pLO,pHI`` (``p0.5,p99.5``) clips every modality of every scan to a pair of its own percentiles over its
own mask as ``prep`` does (pass what the calibration data was prepared with).  The column ``prep_window`` then reads
``p0.5 p99.5`` and ``predict.csv`` gains the column ``window_bounds`` (``lo hi`` per modality, joined by ``;``) after the
``interp`` column's place and before those of ``--blend``.

``--blend gauss`` weighs every window's logits by a Gaussian around the window's centre when the windows are stitched;
``--tta_mirror AXES`` (letters of ``d``, ``h``, ``w``) also runs every window mirrored along each subset of the axes and
averages the logits: 2, 4 or 8 forwards per window.  When either is given ``predict.csv`` gains the columns ``blend`` and
``tta_mirror`` after the others; otherwise the file is what it was.

``--post RULE`` (repeatable; config.post_rules, ``--post_conn 6|26``) cleans the map by connected components on the
scan's own grid before it is counted, copied and written (effq_label_clean): ``--post 1,2:largest`` keeps the largest
component of the labels 1 and 2, ``--post '4:min500>1'`` relabels every component of label 4 with fewer than 500 voxels to
1; ``'1,2:fill>1'`` fills the holes of the mask of the labels 1 and 2 with label 1, ``'1:close2>1'`` closes and
``2:open1`` opens a mask by a ball of that radius in voxels of the scan's grid (effq_label_post).
``predict.csv`` then gains the columns ``post`` (the rules) and ``post_changed`` (the voxels each rule relabelled)
after all others, and ``labels``, ``voxels`` and ``volume_ml`` are the cleaned map's; without ``--post`` nothing changes.

``--thresh VALUE`` (with ``--multi_label``; a probability ``P`` or ``logit:X``, config.parse_thresh) decides every channel
at that threshold instead of sigmoid >= 0.5.  ``predict.csv`` then gains the column ``thresh`` (the fp32 logit, ``%.9g``)
after the blend columns and before the post columns; ``0.5`` and ``logit:0`` are the default and change nothing.

``--save_prob`` also writes ``<out_dir>/prob/<subject>.nii.gz``, uint8 ``(SD, SH, SW, C)`` on the scan's grid with the
scan's header and ``scl_slope`` 1/255: the softmax over the C classes (class-id mode) or the sigmoid of every raw channel
(``--multi_label``; ``--merge_type`` and ``--thresh`` do not enter) of the logits interpolated exactly as for the label
map (effq_seg_probs_source, one call per subject).  ``--save_unc`` writes ``<out_dir>/unc/<subject>.nii.gz``, one uint8
per voxel with the same slope: the entropy over the classes as a share of ln C, or the largest binary entropy of a
channel in bits.  Outside the box the probabilities are the background's (class-id: channel 0 is 255; sigmoid: all 0)
and the uncertainty is 0.  ``--blend`` and ``--tta_mirror`` act through the logits, ``--post`` does not touch these
files, ``predict.csv`` is unchanged, and without the switches nothing changes.

``--lesion_measures`` (``--measure_class LABELS``, ``--measure_plane axial|d|h|w``) measures the uint8 map that is
written, after ``--post`` and on the scan's own grid (ops_measure.label_lesion_measures without a truth map), and writes
``<out_dir>/lesions.csv``: the columns of ``score --lesion_measures`` without ``overlap``, ``kind`` ``pred`` throughout.
The per-subject line gains the lesion count per class; ``predict.csv`` and the maps are unchanged.

Everything the list and the headers decide, a ``--thresh`` that is not understood or given without ``--multi_label``, a ``--post`` rule that is not understood, a ``--blend`` or ``--tta_mirror`` that is not understood, ``--multi_label lits`` (one plane per class has no place on a source grid)
and the choice of the network are refused before anything touches the device or ``out_dir``, in prep's wording.
"""
from __future__ import annotations

import csv
import os
import os.path as P
from contextlib import closing
from types import SimpleNamespace
from typing import List

import numpy as np
import torch

from . import _lib
from . import data as D
from . import evaluate as E
from . import lesion_measures as LM
from . import nifti
from . import prep
from .prep import PrepError

PREDICT_CSV = "predict.csv"
MAX_PENDING_WRITES = 2        # host maps waiting for the writing thread at most
PROB_DIR, UNC_DIR = "prob", "unc"     # under out_dir, made only for --save_prob / --save_unc
PROB_SCALE = (1.0 / 255.0, 0.0)       # scl_slope, scl_inter of both: a reader shows values in [0, 1]
CSV_HEADER = ["subject", "source_shape", "source_spacing", "grid_shape", "pmin", "pmax", "windows", "prep_mask",
              "prep_window", "prep_spacing", "prep_min_size", "patch_size", "labels", "voxels", "volume_ml"]


def _network(args, dev):
    """The network of --resume / --pretrain on `dev`, in the mode it is to run in."""
    from . import calibrate as K
    from . import config as Cf
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    if args.resume:
        return K.load_calibrated(model, args.resume, dev)
    try:
        sd = torch.load(args.pretrain, map_location="cpu")["state_dict"]
    except Exception as e:
        raise SystemExit(f"--pretrain {args.pretrain}: cannot read the checkpoint: {e}")
    if not isinstance(sd, dict):
        raise SystemExit(f"--pretrain {args.pretrain}: its 'state_dict' is no dict of tensors")
    # not strict, as do_ptq loads it (a training checkpoint may carry more than the network); but a checkpoint that
    # fits no key, or leaves a key of the network unset, would segment with random weights: refused, by key
    own = model.state_dict()
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    shapes = [k for k in own if k in sd and tuple(own[k].shape) != tuple(sd[k].shape)]
    if missing or shapes:
        what = (f"{len(missing)} keys of the network are missing, the first {missing[0]}" if missing else
                f"{len(shapes)} shapes differ, the first {shapes[0]}: {tuple(sd[shapes[0]].shape)} in the checkpoint, "
                f"{tuple(own[shapes[0]].shape)} in the network")
        if unexpected:
            what += f"; {len(unexpected)} keys are unexpected, the first {unexpected[0]}"
        raise SystemExit(f"--pretrain {args.pretrain}: the checkpoint does not fit the network of --config: {what}")
    if unexpected:
        print(f"[predict] --pretrain {args.pretrain}: {len(unexpected)} keys of the checkpoint are not the network's "
              f"and are ignored, the first {unexpected[0]}")
    model.load_state_dict(sd, strict=False)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(dev)
    K.set_fp(model)
    return model


CSV_WINDOW_COLUMNS = ["window_bounds"]            # after the interp column's place, only with --prep_window pLO,pHI
CSV_BLEND_COLUMNS = ["blend", "tta_mirror"]       # after CSV_HEADER, only when --blend / --tta_mirror is given
CSV_THRESH_COLUMNS = ["thresh"]                   # after those, only when --thresh is given (and is not the default)
CSV_POST_COLUMNS = ["post", "post_changed"]       # after those, only when --post is given


def _write_csv(path: str, rows: List[dict], header=CSV_HEADER) -> None:
    def dump(p):
        with open(p, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(header)
            w.writerows([r[k] for k in header] for r in rows)
    prep._replace(path, dump)


def _resolve(args, need_network: bool) -> SimpleNamespace:
    """Everything `args`, the list and the headers decide, refused by name before anything touches the device or
    out_dir; returns the mission's job: host values only (`overlap`: the validation's, half a patch at most; `sliding`:
    --blend / --tta_mirror given, their columns are written; `used`: the columns that are the same in every row)."""
    task = (getattr(args, "task", None) or "").lower()
    if task not in D.MODALITIES:
        raise PrepError(f"predict: --task {getattr(args, 'task', None)!r}, one of {', '.join(D.MODALITIES)}")
    if not getattr(args, "src_list", None) or not getattr(args, "out_dir", None):
        raise PrepError("predict: needs --src_list and --out_dir")
    if need_network:
        resume, pretrain = getattr(args, "resume", None), getattr(args, "pretrain", None)
        if bool(resume) == bool(pretrain):
            raise SystemExit(f"predict: needs exactly one of --resume (a calibrated snapshot of the ptq mission) and "
                             f"--pretrain (the FP checkpoint, with --qconv conv), got "
                             f"{'both' if resume else 'neither'}")
        if pretrain and (getattr(args, "qconv", None) or "conv").lower() != "conv":
            raise SystemExit(f"predict: --pretrain is the FP checkpoint and runs with --qconv conv, not --qconv "
                             f"{args.qconv}: a calibrated network is loaded with --resume")
        if resume and not P.isfile(resume):
            raise SystemExit(f"--resume {resume}: no such file")
        if pretrain and not P.isfile(pretrain):
            raise SystemExit(f"--pretrain {pretrain}: no such file")
    multi_label = getattr(args, "multi_label", None)
    try:
        rule = E.label_rule(bool(multi_label), multi_label, task)
    except RuntimeError as e:
        raise PrepError(f"predict: {e}")
    if rule == "planes":
        raise PrepError(f"predict: the maps of --multi_label {multi_label} hold one plane per class (C x D x H x W); a "
                        f"NIfTI image has its spatial axes first, so they cannot be written on the source grid")
    fuse = getattr(args, "merge_type", None) if multi_label else None
    try:
        patch = D.parse_patch(args.patch_size) if getattr(args, "patch_size", None) else D.PATCH_DEFAULT[task]
    except ValueError:
        patch = ()
    if len(patch) != 3 or min(patch) < 1:
        raise PrepError(f"--patch_size {args.patch_size!r}: needs one or three positive integers")
    opts = prep.parse_options(args, task, patch)
    if any(m < p for m, p in zip(opts.min_size, patch)):
        raise PrepError(f"--prep_min_size {tuple(opts.min_size)} is smaller than --patch_size {tuple(patch)}: the sliding "
                        f"window needs one whole patch")
    from . import config as Cf
    blend, flips = Cf.blend_switches(args)
    sliding = (blend, flips) != ("uniform", (0,))
    post, post_conn = Cf.post_rules(args)
    _, thresh = Cf.thr_switches(args, 'predict')
    save_prob, save_unc = Cf.prob_switches(args, 'predict')
    measures = Cf.measure_switches(args, 'predict')
    mods = D.MODALITIES[task]
    plans = [opts.plan(dict(e, seg=None), mods) for e in prep.read_src_list(args.src_list, task)]
    measure = None
    if measures:        # the classes, and per subject the slice axis; the limits of the device call are refused here
        classes = measures[0] or Cf.SCORE_CLASSES[task]
        axes = {}
        for plan in plans:
            shape = tuple(int(n) for n in plan.source_shape)
            if len(classes) * int(np.prod(shape)) >= 2 ** 31 or max(shape) > _lib.EDT_MM_MAX_EXTENT:
                raise PrepError(f"subject {plan.subject}: --lesion_measures: {len(classes)} masks of {prep._fmt(shape)} "
                                f"voxels are outside the limits of the device call (2^31 - 1 voxels in all, every extent "
                                f"at most {_lib.EDT_MM_MAX_EXTENT})")
            axes[plan.subject] = LM.slice_axis(measures[1], plan.affine, plan.subject)
        measure = SimpleNamespace(classes=classes, lut=Cf.score_class_lut(classes), axes=axes)
    window = opts.window
    used = {"prep_mask": opts.mask, "prep_window": str(window) if isinstance(window, prep.PercentileWindow) else
            prep._fmt(window) if window else "none",
            "prep_spacing": prep._fmt(opts.spacing) if opts.spacing else "none",
            "prep_min_size": prep._fmt(opts.min_size), "patch_size": prep._fmt(patch)}
    if sliding:
        used.update(blend=blend, tta_mirror=getattr(args, "tta_mirror", None) or "none")
    if thresh is not None:
        used.update(thresh="%.9g" % thresh)
    post_said = Cf.post_text(post, post_conn) if post else None
    if post:
        used.update(post=post_said)
    return SimpleNamespace(mods=mods, opts=opts, patch=patch, overlap=tuple(min(D.OVERLAP_DEFAULT, p // 2) for p in patch),
                           rule=rule, fuse=fuse, blend=blend, flips=flips, sliding=sliding, post=post, post_conn=post_conn,
                           post_said=post_said, thresh=thresh, save_prob=save_prob, save_unc=save_unc, measure=measure,
                           prob_mode="argmax" if rule == "argmax" else "sigmoid", used=used, plans=plans)


def _on_scan_grid(ops, plan, t):
    """A map `t` of the oriented source grid (D x H x W, or the C planes as N = C volumes; None stays None) back on the
    scan's own grid: one effq_prep_reorient with the inverse plan, nothing when the scan was not turned."""
    if t is None or plan.orient is None or prep.orient_is_identity(*plan.orient):
        return t
    return ops.prep_reorient(t, *prep.orient_inverse(*plan.orient))


def _segment(ops, model, job, plan, imgs, out_dir: str, bsz, write, measures=None):
    """The device work of one subject: its label map and, for --save_prob / --save_unc, its probability and uncertainty
    maps, handed to `write(path, host, geometry, scale=None)`.  Returns (what it leaves for the row and the line, the
    window batch in use): box_of, the extent of the working arrays; counts, the voxels per label value of the map that was
    written; changed, the voxels each --post rule relabelled; extra, what the line says of the probability files."""
    sn = plan.subject
    y, _, _, pmin, pmax, _, _, _ = prep.process_subject(ops, plan, imgs, None, job.mods, job.opts)
    vol = torch.from_numpy(y)[None].to(ops.device)
    outs, nwin, bsz = E.stitched_window_logits(ops, [model], vol, job.patch, job.overlap, bsz, job.blend, job.flips)
    where = (pmin, plan.grid_shape, plan.factors, plan.oriented_shape)
    labels = _on_scan_grid(ops, plan, ops.seg_labels_source(outs[0][0], *where, job.rule, job.fuse))
    changed = None
    if job.post:        # on the source grid, in place: the counts, the copy and the file are the cleaned map's
        labels, stats = ops.label_clean(labels, job.post, job.post_conn, out=labels)
        changed = prep._fmt(int(v) for v in stats.cpu()[:, 1])
    counts = torch.bincount(labels.reshape(-1)).cpu().tolist()      # on the uint8 map itself, before the copy
    lesions = None
    if job.measure:     # of the map that is written: after --post, on the scan's own grid
        m = job.measure
        try:
            _, _, table, meas = measures(labels, None, m.lut, len(m.classes), plan.source_spacing, m.axes[sn])
        except _lib.EffqError as e:
            raise PrepError(f"subject {sn}: --lesion_measures: {e}")
        lesions = LM.lesion_rows(sn, m.classes, False, table, meas, tuple(labels.shape), plan.source_spacing, plan.affine,
                                 m.axes[sn])
    write(P.join(out_dir, f"{sn}.nii.gz"), labels.cpu().numpy(), plan.header)
    extra = ""
    if job.save_prob or job.save_unc:       # from the same stitched logits, on the same grid; --post does not enter
        probs, unc = ops.seg_probs_source(outs[0][0], *where, job.prob_mode, job.save_prob, job.save_unc)
        probs, unc = _on_scan_grid(ops, plan, probs), _on_scan_grid(ops, plan, unc)
        if job.save_prob:       # (C, SD, SH, SW) -> the view (SD, SH, SW, C): a 4-D image, pixdim[4] = 1
            geo = dict(plan.header, pixdim=tuple(plan.header["pixdim"][:4]) + (1.0,) + tuple(plan.header["pixdim"][5:]))
            write(P.join(out_dir, PROB_DIR, f"{sn}.nii.gz"), np.moveaxis(probs.cpu().numpy(), 0, -1), geo, PROB_SCALE)
            extra += f", {PROB_DIR}/{sn}.nii.gz ({probs.shape[0]} channels)"
        if job.save_unc:
            write(P.join(out_dir, UNC_DIR, f"{sn}.nii.gz"), unc.cpu().numpy(), plan.header, PROB_SCALE)
            extra += f", {UNC_DIR}/{sn}.nii.gz"
    return SimpleNamespace(box_of=tuple(y.shape[1:]), pmin=pmin, pmax=pmax, windows=nwin, counts=counts,
                           changed=changed, extra=extra, lesions=lesions), bsz


def _row(job, plan, done) -> dict:
    """The row of predict.csv of one subject."""
    present = [v for v, n in enumerate(done.counts) if n]
    ml = float(np.prod(plan.source_spacing)) / 1000.0
    row = {"subject": plan.subject, "source_shape": prep._fmt(plan.source_shape),
           "source_spacing": prep._fmt(plan.source_spacing), "grid_shape": prep._fmt(plan.grid_shape),
           "pmin": prep._fmt(done.pmin), "pmax": prep._fmt(done.pmax), "windows": str(done.windows),
           "labels": prep._fmt(present), "voxels": prep._fmt(done.counts[v] for v in present),
           "volume_ml": " ".join(f"{done.counts[v] * ml:.7g}" for v in present)}
    row.update(job.used)
    row.update(job.opts.row_values(plan))
    if plan.window_bounds is not None:
        row["window_bounds"] = ";".join(prep._fmt(b) for b in plan.window_bounds)
    if job.post:
        row["post_changed"] = done.changed
    return row


def run(args, ops=None, model=None, window_batch=None, measures=None) -> List[dict]:
    """The `predict` mission of `args` (config.build_parser); returns the rows of predict.csv.  `ops`: the object whose
    prep_*, window_*, seg_labels_source and (for --save_prob / --save_unc) seg_probs_source methods do the device work and whose `device` holds the tensors
    (hip_ops.get_ops(args.device) by default); `model`: the network, already on that device and in its mode (by default
    the one --resume / --pretrain name); `window_batch`: windows per forward (None: sized from the first window's peak
    memory, as validate_seg sizes it); `measures`: the device call of --lesion_measures (ops_measure.label_lesion_measures
    over `ops` by default)."""
    job = _resolve(args, model is None)
    if ops is None:
        from .hip_ops import get_ops
        ops = get_ops(torch.device("cuda", int(getattr(args, "device", 0) or 0)))
    if job.measure and measures is None:
        from functools import partial
        from . import ops_measure as OM
        measures = partial(OM.label_lesion_measures, ops)
    if model is None:
        model = _network(args, ops.device)
    model.eval()

    out_dir = args.out_dir
    os.makedirs(out_dir, exist_ok=True)
    if job.thresh is not None:
        print(f"[predict] --thresh {args.thresh}: every channel is decided at logit >= {job.thresh:.9g} (sigmoid >= "
              f"{E.logit_prob(job.thresh):.6g})")
        ops.set_decision_threshold(job.thresh)
    if job.save_prob or job.save_unc:
        nc = getattr(args, "nClass", None)
        what = " and ".join(w for w, on in ((f"{PROB_DIR}/<subject>.nii.gz (SD, SH, SW, C)", job.save_prob),
                                            (f"{UNC_DIR}/<subject>.nii.gz", job.save_unc)) if on)
        how = (f"softmax over {nc if nc else 'the'} classes, uncertainty = entropy / ln C" if job.prob_mode == "argmax" else
               "sigmoid per channel, uncertainty = the largest binary entropy of a channel in bits")
        print(f"[predict] {what}: {how}, from the logits interpolated as for the label map; uint8 in steps of 1/255 "
              f"(scl_slope), --post does not touch them")
        if job.save_prob and job.prob_mode == "sigmoid" and (job.fuse or job.thresh is not None):
            given = " and ".join(w for w, on in ((f"--merge_type {job.fuse}", job.fuse),
                                                 (f"--thresh {getattr(args, 'thresh', None)}", job.thresh is not None)) if on)
            print(f"[predict] --save_prob: {given} decide the label map only: the probabilities are the network's, per "
                  f"raw channel, not a decision's")
        for on, sub in ((job.save_prob, PROB_DIR), (job.save_unc, UNC_DIR)):
            if on:
                os.makedirs(P.join(out_dir, sub), exist_ok=True)
    rows, lesions = [], []
    bsz = window_batch
    try:
        with nifti.BackgroundWriter("effq-predict-write", MAX_PENDING_WRITES) as writer, \
                closing(prep.read_subjects(job.plans, job.mods, "effq-predict-read")) as subjects:
            def write(path, host, geometry, scale=None):
                writer.submit(nifti.write_nifti, path, host, None, geometry, scale)
            for plan, imgs, _ in subjects:
                done, bsz = _segment(ops, model, job, plan, imgs, out_dir, bsz, write, measures)
                rows.append(_row(job, plan, done))
                cleaned = f", post {job.post_said}: {done.changed} voxels relabelled" if job.post else ""
                if job.measure:
                    lesions += done.lesions
                    cleaned += ", lesions " + ", ".join(
                        f"class {c} ({prep._fmt(labels)}): {sum(1 for r in done.lesions if r['class'] == c)}"
                        for c, labels in enumerate(job.measure.classes))
                print(f"[predict] {plan.subject}: {prep._fmt(plan.source_shape)}{job.opts.said(plan, job.mods)} -> grid "
                      f"{prep._fmt(plan.grid_shape)}, box at {prep._fmt(done.pmin)} of {prep._fmt(done.box_of)}, "
                      f"{done.windows} windows{f' x {len(job.flips)} passes, blend {job.blend}' if job.sliding else ''}, "
                      f"labels {rows[-1]['labels']}: {rows[-1]['voxels']} voxels{cleaned}{done.extra}")
    finally:
        if job.thresh is not None:
            ops.set_decision_threshold(None)
    pct = isinstance(job.opts.window, prep.PercentileWindow)
    _write_csv(P.join(out_dir, PREDICT_CSV), rows,
               CSV_HEADER + job.opts.columns() + (CSV_WINDOW_COLUMNS if pct else []) +
               (CSV_BLEND_COLUMNS if job.sliding else []) +
               (CSV_THRESH_COLUMNS if job.thresh is not None else []) + (CSV_POST_COLUMNS if job.post else []))
    if job.measure:
        LM.write_csv(P.join(out_dir, LM.LESIONS_CSV), [k for k in LM.LESION_COLUMNS if k != "overlap"], lesions)
        print(f"[predict] {len(lesions)} lesions measured: {P.join(out_dir, LM.LESIONS_CSV)}")
    print(f"[predict] {len(rows)} maps written to {out_dir}")
    return rows
