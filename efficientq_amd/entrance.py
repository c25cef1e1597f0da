"""Command-line entry of the ``ptq`` mission, same surface as the reference's ``src/entrance.py``
(`python entrance.py ptq --qlvl_w 4 --qlvl_a 4 --round 1 --config ../config/brats_ptq.yaml --pretrain ...`):

    python -m efficientq_amd.entrance ptq --config config/brats_ptq.yaml --qlvl_w 4 --qlvl_a 4 \
        --pretrain pretrain/brats/round1/mid/state_0500.pkl --synthetic --lwq_batchsz 2 --snap_dir out/

Labelled volumes in the reference's layout are read with ``--data_dir`` / ``--split_dir`` (data.py): the
calibration takes the train split, and ``--test_fp`` / the default test (unless ``--no_test``) validate the FP and
the calibrated network on the val split (evaluate.validate_seg), writing ``<snap>/{fp,ptq}/metrics.csv``;
``--save_nii`` adds the predicted label maps ``<snap>/{fp,ptq}/val/<subject>.nii.gz`` and ``<snap>/{Q,FP}seg<i>.nii.gz``;
``--is_cc`` adds the lesion-level columns ``totall, predl, fnl, fpl`` (connected components) to ``metrics.csv``;
``--surf_dist`` adds the surface distances ``hd, hd95, assd`` (voxel units) after them;
``--lesion_table`` writes ``<snap>/{fp,ptq}/lesions.csv``, one row per label lesion and per predicted lesion (first
voxel, size, overlap; ``vol_mm3`` with ``--src_geom`` / ``--spacing``), and prints the detected lesions per size bin;
``--lesion_match`` matches label lesions and predicted lesions one to one at IoU > 0.5 from the overlap of every pair of
them (effq_seg_lesion_match): ``<snap>/{fp,ptq}/lesion_match.csv`` (per subject and class ``tp_l, fp_l, fn_l, f1_l, sq,
pq, lw_dsc, groups``) and ``lesion_pairs.csv`` (every pair of overlapping lesions with its overlap and IoU), with
``--lesion_table`` also the columns ``match, best_iou, partners`` of ``lesions.csv``; it needs labels and a validation;
``--src_geom`` reads every val subject's source image header (``data_dir/sn_fn.txt``, data.py): the distances become
``hd_mm, hd95_mm, assd_mm`` in millimetres and the val maps are written on the source grid with the source's geometry;
``--spacing d,h,w`` gives the distances in millimetres from one spacing for all subjects, without any file.
``--vs_fp`` validates the calibrated network against the network it was calibrated from (a copy taken before the
calibration): ``<snap>/ptq/agreement.csv`` with, per subject and class, the FP-vs-Q Dice and counts, the share of voxels
decided differently, the logit drift and the probability drift, the lesion / surface columns of ``--is_cc`` /
``--surf_dist`` against the FP decisions, and with ``--save_nii`` the map of the differing classes
``<snap>/ptq/val_vs_fp/<subject>.nii.gz``; it needs no label;
``--unlabelled`` (with ``--vs_fp``) reads data without a ``seg/`` folder: only the FP-vs-Q validation runs.
``--blend gauss`` weighs every window's logits by a Gaussian around the window's centre when the windows are stitched, and
``--tta_mirror AXES`` (letters of ``d``, ``h``, ``w``) also runs every window mirrored along each subset of the axes and
averages the logits; both hold for every validation of the run (and for ``predict``), the FP network's included.
``--post RULE`` (repeatable, ``--post_conn 6|26``) also cleans every labelled val case's predicted map by connected
components on the device (``1,2:largest`` keeps the largest component of the labels 1 and 2, ``'4:min500>1'`` - quoted,
or the shell takes ``>1`` for a redirection - relabels every component of label 4 with fewer than 500 voxels to 1;
``'1,2:fill>1'`` fills the holes of the mask of the labels 1 and 2 with 1, ``'1:close2>1'`` closes and ``2:open1`` opens a
mask by a ball of that radius in voxels: effq_label_post) and scores the cleaned map:
``<snap>/{fp,ptq}/metrics_post.csv``; ``metrics.csv`` and every other file stay what they are.
It needs labels: with ``--unlabelled`` or ``--synthetic`` it is refused.  ``predict --post`` writes the cleaned maps.
``--thr_sweep`` also sweeps the decision threshold of every labelled validation in one more pass over the stitched logits
(effq_seg_sweep): ``<snap>/{fp,ptq}/threshold.csv`` (per subject and class, and pooled: the ROC AUC, the Dice at the default
decision, the threshold of the best Dice and the Dice, sensitivity and specificity there) and ``threshold_curve.csv`` (the
pooled counts and Dice of every threshold), and per class the mean AUC and the pooled Dice at the default and at the best
threshold, with ``--test_fp`` for both networks side by side; it needs labels and a validation: with ``--unlabelled``,
``--synthetic`` or ``--no_test`` it is refused.  ``--thresh P`` / ``--thresh logit:X`` (with ``--multi_label``) takes every
sigmoid decision of the run, for both networks, at that threshold instead of 0.5 (``predict`` takes it too).
``--synthetic`` instead calibrates on seeded synthetic volumes (``synth.py``) and validates nothing, unless ``--vs_fp``
is given: then two held-out synthetic volumes are validated against the FP network; without
``--pretrain`` a seeded random-init network stands in for the checkpoint.  With ``torchrun --nproc-per-node N``
the calibration volumes are sharded over N GPUs and the validation runs on rank 0.

The ``prep`` mission (prep.py) writes that layout from source NIfTI scans:

    python -m efficientq_amd.entrance prep --task brats --src_list cases.csv --data_dir out/data --split_dir out/split \
        --val_every 5

The ``predict`` mission (predict.py) segments new scans with a snapshot the ``ptq`` mission wrote (``--resume``, loaded by
calibrate.load_calibrated) or with the FP checkpoint (``--pretrain --qconv conv``), and writes one uint8 label map per
subject on the scan's own grid, with the scan's header, and ``predict.csv``:

    python -m efficientq_amd.entrance predict --config config/lits_ptq.yaml --qlvl_w 4 --qlvl_a 4 \
        --resume out/state_in_fp.pkl --src_list new_cases.csv --out_dir seg/

The ``score`` mission (score.py) scores finished label maps - those of ``predict``, or of any other tool - against the
``seg`` column of the same list, on the scan's own grid: Dice, lesion counts, surface distances in millimetres and the
normalised surface Dice at ``--score_tol`` per subject and class in ``score/scores.csv``, the means in ``summary.csv``:

    python -m efficientq_amd.entrance score --task lits --src_list cases.csv --pred_dir seg/ --out_dir score/ \
        --score_tol 1,3
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

from . import calibrate as K
from . import config as Cf
from . import data as D
from . import evaluate as E
from . import reports as R
from . import synth


class _SnapshotWriter:
    """Stand-in for the reference's PTQTester (utils/tester.py:37-51): the three snapshot files only."""

    def __init__(self, model, root):
        self.model, self.root = model, root

    def test_as_is(self, *a, **k):
        print('[entrance] evaluation (sliding-window Dice) is outside the calibrated hot path: skipped')

    def snapshot(self, name, compress=False):
        sd = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        path = os.path.join(self.root, name)
        if compress:
            np.savez_compressed(path, **{k: v.numpy() for k, v in sd.items()})
        else:
            torch.save({'state_dict': sd}, path)
        print(f'[entrance] wrote {path}')


class _ValidationTester(_SnapshotWriter):
    """The reference's PTQTester on labelled data: test_as_is validates on the val split (rank 0 only) and writes
    <root>/<folder>/metrics.csv, with is_save_nii also every val subject's predicted map as
    <root>/<folder>/val/<subject>.nii.gz (trainer.validate_final), with is_cc also the lesion-level columns, with is_surf also the
    surface distances, with is_table also <root>/<folder>/lesions.csv, with is_match also lesion_match.csv and
    lesion_pairs.csv there, with fp_model (--vs_fp) also
    <root>/<folder>/agreement.csv and, with is_save_nii, <root>/<folder>/val_vs_fp/<subject>.nii.gz.  On a cube without
    labels (--unlabelled, --synthetic --vs_fp) only the validation against fp_model runs and metrics.csv is not written.
    With sweep (--thr_sweep) also <root>/<folder>/threshold.csv and threshold_curve.csv.  What it prints is
    formatted by reports.py."""

    def __init__(self, model, root, data_cube, task, rank=0, blend='uniform', flips=(0,), post=(), post_conn=26,
                 sweep=False):
        super().__init__(model, root)
        self.cube, self.task, self.rank = data_cube, task.lower(), rank
        self.blend, self.flips = blend, tuple(flips)
        self.post, self.post_conn = list(post), post_conn
        self.sweep, self.swept = bool(sweep), {}           # swept: folder -> (mean AUC per class, pooled summary)

    def _geometry(self, is_save_nii, is_surf, is_table=False):
        """validate_seg's `geometry`, only when a switch asks for one: the per-subject entries of --src_geom (distances,
        lesion volumes and maps), or the one spacing of --spacing (distances and lesion volumes only)."""
        geom = getattr(self.cube, 'geometry', None)
        if geom is not None and (is_save_nii or is_surf or is_table):
            return geom
        spacing = getattr(self.cube, 'spacing', None)
        return spacing if spacing is not None and (is_surf or is_table) else None

    def test_as_is(self, folder='results', is_save_nii=False, is_cc=False, is_surf=False, is_table=False,
                   fp_model=None, is_match=False):
        if self.rank != 0:
            return
        if self.cube.valloader is None:
            print('[entrance] no val split: validation skipped')
            return
        out = os.path.join(self.root, folder)
        labelled = getattr(self.cube, 'labelled', True)
        if not labelled and fp_model is None:
            print(f'[entrance] {folder}: the val cases have no labels: validation skipped')
            return
        t0 = time.time()
        res = E.validate_seg(self.model, self.cube.valloader, self.task, self.cube.patch_size, self.cube.overlap,
                             fuse=self.cube.multilabel_fusetype, names=self.cube.val_sn,
                             save_dir=os.path.join(out, 'val') if is_save_nii else None,
                             multi_label=getattr(self.cube, 'multi_label', None), lesions=is_cc, surface=is_surf,
                             geometry=self._geometry(is_save_nii, is_surf, is_table), lesion_table=is_table,
                             fp_model=fp_model, blend=self.blend, flips=self.flips, post=self.post,
                             post_conn=self.post_conn, sweep=self.sweep and labelled,
                             lesion_match=is_match and labelled)
        os.makedirs(out, exist_ok=True)
        if fp_model is not None:
            E.write_agreement_csv(os.path.join(out, 'agreement.csv'), res)
        if not labelled:
            print(f'[entrance] {folder}: {len(res)} unlabelled val cases in {time.time() - t0:.2f}s')
            print('\n'.join(R.agreement_lines(folder, res)))
            return
        E.write_metrics_csv(os.path.join(out, 'metrics.csv'), res)
        if is_table:
            E.write_lesions_csv(os.path.join(out, 'lesions.csv'), res)
        if is_match:
            from . import lesion_match as LM
            LM.write_lesion_match_csv(os.path.join(out, 'lesion_match.csv'), res)
            LM.write_lesion_pairs_csv(os.path.join(out, 'lesion_pairs.csv'), res)
        lines = R.metric_lines(folder, res, time.time() - t0, is_cc, is_surf)
        if is_table:
            lines += R.lesion_size_lines(folder, res)
        if is_match:
            lines += R.lesion_match_lines(folder, res)
        if self.post:
            E.write_metrics_post_csv(os.path.join(out, 'metrics_post.csv'), res)
            lines += R.post_lines(folder, res, Cf.post_text(self.post, self.post_conn), len(self.post))
        if self.sweep:          # every network swept so far side by side
            E.write_threshold_csv(os.path.join(out, 'threshold.csv'), res)
            E.write_threshold_curve_csv(os.path.join(out, 'threshold_curve.csv'), res)
            self.swept[folder] = R.sweep_means(res)
            lines += R.sweep_lines(folder, self.swept, bool(getattr(self.cube, 'multi_label', None)))
        if fp_model is not None:
            lines += R.agreement_lines(folder, res)
        print('\n'.join(lines))


class _SyntheticCube:
    """The calibration volumes of --synthetic; with `validate` (--vs_fp) also two held-out volumes without labels, each
    one window of the calibration size."""
    valloader = None

    def __init__(self, task, n, size, validate=False, multi_label=None):
        vols = synth.calib_batch(task, range(n), size)

        class DS(torch.utils.data.Dataset):
            def __len__(self):
                return n

            def __getitem__(self, i):
                return vols[i], torch.zeros(vols.shape[2:], dtype=torch.long)

            def use_fix_transform(self):
                pass
        self.trainseqloader = torch.utils.data.DataLoader(DS(), 1, shuffle=False)
        if validate:
            held = synth.calib_batch(task, [n, n + 1], size)
            self.valloader = [(v[None], torch.empty(1, 0, dtype=torch.uint8)) for v in held]
            self.val_sn = [f'synth{n}', f'synth{n + 1}']
            self.labelled = False
            self.patch_size, self.overlap = tuple(held.shape[2:]), 0
            self.multi_label, self.multilabel_fusetype = multi_label, None


def _switches(args):
    """The switch families of the ptq mission, each parsed and checked once, before anything touches the device (host
    only: SystemExit naming the switches): ((blend, flips), (post rules, connectivity), (sweep, thresh), lesion_match)."""
    sliding = Cf.blend_switches(args)
    post = check_post(args)
    thr = Cf.thr_switches(args)
    Cf.prob_switches(args)
    match = Cf.match_switches(args)
    Cf.score_switches(args, 'ptq')
    Cf.measure_switches(args, 'ptq')
    if getattr(args, 'unlabelled', False):
        if not getattr(args, 'vs_fp', False):
            raise SystemExit('--unlabelled: without labels only the validation against the FP network can run: add '
                             '--vs_fp')
        if getattr(args, 'test_fp', False):
            raise SystemExit('--unlabelled --test_fp: the FP network cannot be validated against labels that are not '
                             'there: drop --test_fp')
        if getattr(args, 'lesion_table', False):
            raise SystemExit('--unlabelled --lesion_table: the per-lesion table is written against labels only (--is_cc '
                             'and --surf_dist are measured against the FP network): drop --lesion_table')
    return sliding, post, thr, match


def check_switches(args):
    """The combinations of --vs_fp / --unlabelled that cannot run and the values of --blend / --tta_mirror that are not
    understood, refused before anything touches the device (host only: SystemExit naming the switches)."""
    _switches(args)


def check_post(args):
    """The --post rules that are not understood and the missions and label forms they cannot serve, refused by name
    before anything runs (host only: SystemExit); returns (rules, connectivity)."""
    rules, conn = Cf.post_rules(args)
    if not rules:
        return rules, conn
    if getattr(args, 'mission', None) == 'prep':
        raise SystemExit('--post cleans predicted label maps: the prep mission predicts nothing, drop --post')
    multi_label = getattr(args, 'multi_label', None)
    if multi_label:
        rule = E.label_rule(True, multi_label, (getattr(args, 'task', None) or 'lits').lower())
        if rule == 'planes' or not getattr(args, 'merge_type', None):
            raise SystemExit(E.post_refusal(rule))
    for switch in ('unlabelled', 'synthetic'):
        if getattr(args, switch, False):
            raise SystemExit(f'--post --{switch}: a cleaned map is scored against the labels, and there are none: drop '
                             f'--post (the predict mission cleans maps without labels)')
    return rules, conn


def main(argv=None):
    args = Cf.build_parser().parse_args(argv)
    if args.config:
        args = Cf.merge_config(args.config, args)
    if args.mission == 'prep':
        check_post(args)
        Cf.thr_switches(args)
        Cf.prob_switches(args)
        Cf.match_switches(args)
        Cf.score_switches(args)
        Cf.measure_switches(args)
        from . import prep
        prep.run(args)
        return
    if args.mission == 'predict':       # refused ahead of predict.run's own checks, which hold for a direct caller too
        Cf.thr_switches(args)
        Cf.match_switches(args)
        Cf.score_switches(args)
        from . import predict
        predict.run(args)
        return
    if args.mission == 'score':         # score.run refuses the switches of the other missions itself (score_switches)
        from . import score
        score.run(args)
        return
    if args.mission != 'ptq':
        raise NotImplementedError(args.mission)
    (blend, flips), (post, post_conn), (sweep, thresh), match = _switches(args)
    if (blend, flips) != ('uniform', (0,)):
        print(f'[entrance] sliding window: blend {blend}, {len(flips)} passes per window (flip masks '
              f'{" ".join(str(m) for m in flips)})')
    if post:
        print(f'[entrance] --post {Cf.post_text(post, post_conn)}: every labelled validation also scores the cleaned map '
              f'(metrics_post.csv)')
    if sweep:
        print('[entrance] --thr_sweep: every labelled validation also sweeps the decision threshold (threshold.csv, '
              'threshold_curve.csv)')
    if match:
        print('[entrance] --lesion_match: every labelled validation also matches its lesions one to one '
              '(lesion_match.csv, lesion_pairs.csv)')
    tester_kw = dict(blend=blend, flips=flips, post=post, post_conn=post_conn, sweep=sweep)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        torch.cuda.set_device(local)
        # (no device_id: the group is the rendezvous only; the collectives are RCCL calls on the kernels' stream, rccl.py -
        # an eagerly created framework communicator brings streams of its own that slow the calibration by 20 %)
        dist.init_process_group('nccl')
        args.device = local
    if thresh is None:
        return _ptq(args, tester_kw)
    from .hip_ops import get_ops
    ops = get_ops(torch.device('cuda', int(args.device)))
    print(f'[entrance] --thresh {args.thresh}: every channel is decided at logit >= {thresh:.9g} (sigmoid >= '
          f'{E.logit_prob(thresh):.6g}) in every validation and map of this run, for both networks alike')
    ops.set_decision_threshold(thresh)
    try:
        return _ptq(args, tester_kw)
    finally:
        ops.set_decision_threshold(None)


def _ptq(args, tester_kw):
    """The ptq mission after its switches are checked: `tester_kw` are the keywords of the _ValidationTester."""
    QConv, Qinfo, kwQ = Cf.get_conv_class(args)
    cube, info = Cf.get_model_cube(args, QConv, kwQ)
    model = cube['model']
    snap = args.snap_dir or os.path.join('exp_ptq', args.task, f'{info}_{time.strftime("%m%d%H%M")}_{Qinfo}{args.suffix}')
    os.makedirs(snap, exist_ok=True)
    if not args.pretrain:
        synth.randomise_network(model, 0)
        args.pretrain = os.path.join(snap, 'round%s_random_init.pkl' % args.round)
        torch.save({'state_dict': model.state_dict()}, args.pretrain)
        cube['pretrain'] = args.pretrain
        print(f'[entrance] no --pretrain given: seeded random-init network saved to {args.pretrain}')
    if args.synthetic:
        size = [int(v) for v in args.lwq_patchsz.split(',')] if args.lwq_patchsz else (128 if args.task == 'brats' else 160)
        size = size[0] if isinstance(size, list) and len(set(size)) == 1 else size
        data_cube = _SyntheticCube(args.task, args.lwq_batchsz, size, getattr(args, 'vs_fp', False),
                                   getattr(args, 'multi_label', None))
    else:
        if not (args.data_dir and args.split_dir):
            raise SystemExit('no dataset is shipped: pass --data_dir and --split_dir, or --synthetic')
        data_cube = D.get_data_cube(args)
        if args.save_nii and data_cube.geometry is not None and data_cube.multi_label and \
                E.label_rule(True, data_cube.multi_label, args.task) == 'planes':
            raise SystemExit(f'--save_nii --src_geom: the maps of --multi_label {data_cube.multi_label} hold one plane '
                             f'per class (C x D x H x W) and cannot be written on the source grid of '
                             f'{", ".join(data_cube.val_sn)}: drop --src_geom (or --save_nii)')
    with open(os.path.join(snap, 'cmd.txt'), 'w') as f:
        f.write(' '.join(sys.argv) + '\n')
    if args.synthetic and data_cube.valloader is None:      # nothing to validate: the snapshot files only
        tester = _SnapshotWriter(model, snap)
    else:
        tester = _ValidationTester(model, snap, data_cube, args.task, int(os.environ.get('RANK', '0')), **tester_kw)
    K.do_ptq(args, cube, data_cube, tester, snap)


if __name__ == '__main__':
    main()
