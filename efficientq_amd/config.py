"""CLI / YAML surface of the missions (``prep``: prep.py, ``predict``: predict.py, ``score``: score.py) and factories of the ``ptq`` mission, same flag names and semantics as the
reference (src/entrance.py:17-128, src/definer.py:130-248,286-329): YAML values override the
command line for every non-null key (quirk Q15); ``qlvl_*`` are LEVEL counts (4 => 2-bit);
``q_first/q_last "W,A"`` with A=-1 => full-precision activations (quirk Q14); every ``lwq_*``
argument is forwarded to the conv constructor as ``**kwQ``.
``--qconv effq`` (and the explicit alias ``effq_hip``) selects the MI355X calibrator."""
from __future__ import annotations

import argparse
import collections
import re

import torch.nn as nn
import yaml

from .qconv import EfficientQConvHIP
from .unet import UResQ

QCONV_REGISTRY = {'conv': nn.Conv3d, 'effq': EfficientQConvHIP, 'effq_hip': EfficientQConvHIP}


def merge_config(cfg: str, args: argparse.Namespace):
    with open(cfg, 'r') as fid:
        config = yaml.load(fid, Loader=yaml.FullLoader)
    for k, v in config.items():
        if v is not None:
            setattr(args, k, v)
    return args


def build_parser():
    p = argparse.ArgumentParser(description='EfficientQ PTQ calibration on MI355X')
    p.add_argument('mission', choices=['ptq', 'prep', 'predict', 'score'])
    p.add_argument('--pretrain')
    p.add_argument('--resume')
    p.add_argument('--device', default=0, type=int, help='GPU ID.')
    p.add_argument('--task')
    p.add_argument('--suffix', default="", type=str)
    p.add_argument('--test_fp', action='store_true')
    p.add_argument('--config', type=str)
    p.add_argument('--data_dir')
    p.add_argument('--split_dir')
    p.add_argument('--access_type', default='npy', choices=['npy', 'npz'])
    p.add_argument('--merge_type', help='how to merge multiple labels (agg / con)')
    p.add_argument('--round', default='1', type=str)
    p.add_argument('--patch_size')
    p.add_argument('--bin_label')
    p.add_argument('--multi_label')
    p.add_argument('--model', default='UResQ')
    p.add_argument('--nMod', type=int)
    p.add_argument('--nClass', type=int)
    p.add_argument('--init_stride', type=str, default='1')
    p.add_argument('--depth')
    p.add_argument('--width')
    p.add_argument('--dilation')
    p.add_argument('--nla', default='relu')
    p.add_argument('--norm', type=str, default='bn')
    p.add_argument('--drop_rate', default=0.2, type=float)
    p.add_argument('--ds', type=str, default=None, choices=['simple', 'complex', ''])
    p.add_argument('--init_kernel', default=3, type=int)
    p.add_argument('--hetero_dim', action='store_true')
    p.add_argument('--blk', type=str, default='pre')
    p.add_argument('--no_test', action='store_true')
    p.add_argument('--qconv', default='conv')
    p.add_argument('--qlvl_w', type=int)
    p.add_argument('--qlvl_a', type=int)
    p.add_argument('--q_first')
    p.add_argument('--q_last')
    p.add_argument('--debug', action='store_true')
    p.add_argument('--lwq_dataid', type=int, default=0)
    p.add_argument('--lwq_batchsz', type=int, default=1)
    p.add_argument('--lwq_patchsz')
    p.add_argument('--lwq_verbose', action='store_true')
    # new in this build: one weight scale per output channel (the reference's alpha_w is one scalar per layer)
    p.add_argument('--lwq_channel_wise', action='store_true')
    p.add_argument('--save_nii', action='store_true')
    p.add_argument('--is_cc', action='store_true', help='lesion-level metrics from connected components')
    p.add_argument('--surf_dist', action='store_true', help='surface distances hd, hd95, assd (voxel units)')
    p.add_argument('--lesion_table', action='store_true',
                   help='one row per lesion (first voxel, size, overlap) in <snap>/{fp,ptq}/lesions.csv')
    p.add_argument('--lesion_match', action='store_true',
                   help='ptq: match label lesions and predicted lesions one to one at IoU > 0.5: lesion F1, panoptic '
                        'quality and lesion-wise Dice in <snap>/{fp,ptq}/lesion_match.csv, the overlapping pairs in '
                        'lesion_pairs.csv; refused combinations are named by match_switches')
    p.add_argument('--vs_fp', action='store_true',
                   help='validate the calibrated network against the FP network: <snap>/ptq/agreement.csv')
    p.add_argument('--unlabelled', action='store_true',
                   help='the data has no seg/ labels: validation against the FP network only (needs --vs_fp)')
    p.add_argument('--src_geom', action='store_true',
                   help="take every val subject's affine, spacing and shape from the image sn_fn.txt names: surface "
                        "distances in mm, label maps on the source grid")
    p.add_argument('--spacing', default=None, help='d,h,w in mm for all subjects: surface distances in mm')
    # new in this build: synthetic calibration volumes (no dataset is shipped with either repo)
    p.add_argument('--synthetic', action='store_true', help='calibrate on seeded synthetic volumes')
    p.add_argument('--snap_dir', default=None)
    # the prep mission (prep.py): source NIfTI scans to the data layout --data_dir / --split_dir name
    p.add_argument('--src_list', default=None, help='prep: CSV `subject,<modality>,...[,seg]` of NIfTI paths')
    p.add_argument('--val_every', default=None, type=int,
                   help='prep, with --split_dir: every K-th of the sorted subjects goes to val.txt, the rest to train.txt')
    p.add_argument('--prep_mask', default=None, choices=['nonzero', 'all'],
                   help='prep: the voxels a modality is standardised over (brats: nonzero, lits: all)')
    p.add_argument('--prep_window', default=None, help='prep, predict: lo,hi to clip to first (lits: -200,250), pLO,pHI (p0.5,p99.5) to clip every '
                        'modality inside its mask to its own percentiles over that mask, or none')
    p.add_argument('--prep_orient', default=None,
                   help='prep, predict: three letters, one each of R/L, A/P, S/I (RAS, LPS, SAR, ...): the anatomical '
                        'direction array axis 0, 1, 2 of the working arrays runs towards; every scan is reoriented to it')
    p.add_argument('--prep_spacing', default=None, help='prep: d,h,w in mm to resample every subject to')
    p.add_argument('--prep_antialias', action='store_true',
                   help='prep, predict, with --prep_spacing: a Gaussian over the images before they are down-sampled, per '
                        'axis of factor f > 1 with sigma = (f - 1) / 2 voxels of the source grid (truncated at 4 sigma)')
    p.add_argument('--prep_interp', default='linear',
                   help='prep, predict: linear (trilinear, the default) or cubic (with --prep_spacing): the images are '
                        'resampled by cubic B-spline interpolation, as scipy and skimage do at order=3 with mode mirror; '
                        'the label stays nearest')
    p.add_argument('--prep_align', default=None, metavar='MODALITY',
                   help='prep, predict: the reference modality; every other modality (and the label) whose header lies '
                        'on another grid is resampled onto the reference\'s grid by the affines as they stand '
                        '(trilinear, the label nearest); no registration')
    p.add_argument('--prep_min_size', default=None, help='prep: d,h,w, the least extent of a crop (the task\'s patch)')
    p.add_argument('--prep_no_crop', action='store_true', help='prep: keep the whole grid')
    # the predict mission (predict.py): label maps of new scans from a snapshot (--resume) or the FP checkpoint
    p.add_argument('--out_dir', default=None, help='predict: where <subject>.nii.gz and predict.csv are written')
    # the sliding window of the validation (ptq) and of predict: window weights and mirror test-time augmentation; the
    # values are checked by blend_switches, after the YAML has been merged in
    p.add_argument('--blend', default='uniform', help='window weights of the stitch: uniform or gauss (sigma = patch / 8)')
    p.add_argument('--tta_mirror', default=None,
                   help='mirror test-time augmentation: letters of d, h, w, each at most once (w, hw, dhw); every '
                        'window also runs mirrored along each subset of the axes and the logits are averaged')
    # connected-component clean-up of the predicted label maps (predict, and the validation of ptq); the rules are checked
    # by post_rules, after the YAML has been merged in
    p.add_argument('--post', action='append', default=None, metavar='RULE',
                   help='clean the predicted map by connected components, repeatable, in order: LABELS:largest[>TO] keeps '
                        'the largest component of the voxels whose label is one of LABELS, LABELS:minN[>TO] relabels '
                        'every component of fewer than N voxels; the others become TO (default 0): 1,2:largest  \'4:min500>1\' '
                        '(quote a rule with > on a shell command line: unquoted, the shell takes >TO for a redirection).  '
                        'LABELS:fill[>TO] fills the holes of the mask (enclosed voxels of any other label included), '
                        'LABELS:closeR[>TO] closes it by a ball of R voxels (1 to 32): the added voxels become TO, one of '
                        'LABELS (default the first); LABELS:openR[>TO] opens it: the removed voxels become TO (default '
                        '0): \'1,2:fill>1\'  2:open1')
    p.add_argument('--post_conn', default=None, help='the neighbourhood of every --post rule: 26 (default) or 6')
    # the threshold sweep of the validation and the decision threshold of a run; refused combinations and values are
    # named by thr_switches, after the YAML has been merged in
    p.add_argument('--thr_sweep', action='store_true',
                   help='ptq: sweep the decision threshold of every validation: ROC AUC, the best-Dice threshold and the '
                        'pooled curve in <snap>/{fp,ptq}/threshold.csv and threshold_curve.csv')
    p.add_argument('--thresh', default=None, metavar='VALUE',
                   help='ptq, predict, with --multi_label: decide every channel at this threshold instead of sigmoid >= '
                        '0.5: a probability P (0 < P < 1) or logit:X')
    # the probabilities behind the label maps of predict; refused by name in the other missions (prob_switches)
    p.add_argument('--save_prob', action='store_true',
                   help='predict: also write <out_dir>/prob/<subject>.nii.gz, the probability of every class (softmax) or '
                        'raw channel (sigmoid, with --multi_label) on the scan\'s grid: uint8 (SD, SH, SW, C), scl_slope '
                        '1/255')
    p.add_argument('--save_unc', action='store_true',
                   help='predict: also write <out_dir>/unc/<subject>.nii.gz, one uncertainty per voxel of the scan\'s grid '
                        '(entropy as a share of its maximum): uint8, scl_slope 1/255')
    # the score mission (score.py): finished label maps against the labels of --src_list, on the scan's grid; the values
    # are checked by score_switches, after the YAML has been merged in
    p.add_argument('--pred_dir', default=None, help='score: the folder of the maps <subject>.nii.gz (or .nii) to score')
    p.add_argument('--score_class', action='append', default=None, metavar='LABELS',
                   help='score: one class per switch, repeatable (at most 8): the voxels whose value is one of LABELS '
                        '(1 to 255, comma separated); brats: 1,2,4  1,4  4 (WT, TC, ET), lits: 1,2  2 (liver, tumour)')
    p.add_argument('--score_tol', default=None, metavar='T[,T...]',
                   help='score: the tolerances in mm of the normalised surface Dice (at most 8, default 1), one column '
                        'nsd_<T>mm each; none: no such column')
    # one record per lesion of the maps of score and predict; the values and the missions are checked by measure_switches,
    # after the YAML has been merged in
    p.add_argument('--lesion_measures', action='store_true',
                   help='score, predict: one row per lesion in <out_dir>/lesions.csv: place, volume in ml, centroid in '
                        'scanner coordinates, box, the longest diameter in mm in 3-D and inside one slice; score also '
                        'writes the detection rate by diameter in <out_dir>/lesion_detect.csv')
    p.add_argument('--measure_class', action='append', default=None, metavar='LABELS',
                   help='predict, with --lesion_measures: one class per switch as --score_class (at most 8; default the '
                        'classes of the task); score measures the classes of --score_class')
    p.add_argument('--measure_plane', default=None, metavar='axial|d|h|w',
                   help='with --lesion_measures: the slices of the in-plane diameter: axial (default; the array axis '
                        'nearest to world z by the header) or the array axis they are stacked along')
    # `--prep_window -200,250`: argparse takes a value that starts with `-` for a switch unless it looks like a negative
    # number, and its own pattern knows no comma
    p._negative_number_matcher = re.compile(r'^-\d[\d.,eE+-]*$')
    return p


def blend_switches(args):
    """(blend, flips) of --blend / --tta_mirror (or the YAML keys `blend`, `tta_mirror`) for
    evaluate.stitched_window_logits; a value that is not understood is refused by name (SystemExit), host only."""
    from .evaluate import BLEND_KINDS, mirror_flips
    blend = getattr(args, 'blend', None)
    blend = 'uniform' if blend is None else blend
    if blend not in BLEND_KINDS:
        raise SystemExit(f'--blend {blend!r}: one of {", ".join(BLEND_KINDS)}')
    try:
        flips = mirror_flips(getattr(args, 'tta_mirror', None))
    except ValueError as e:
        raise SystemExit(f'--tta_mirror {e}')
    return blend, flips


def parse_thresh(value):
    """The fp32 logit of a --thresh VALUE: `P` with 0 < P < 1 is a probability and gives the fp32 nearest
    log(P / (1 - P)) in fp64, `logit:X` the fp32 nearest X.  None for 0.5 and logit:0, the default decision.  What is
    not understood is refused by name (SystemExit)."""
    import math
    import numpy as np
    t = str(value).strip()
    is_logit = t.lower().startswith('logit:')
    try:
        x = float(t[6:] if is_logit else t)
    except ValueError:
        raise SystemExit(f'--thresh {t!r}: a probability P with 0 < P < 1, or logit:X')
    if not math.isfinite(x):
        raise SystemExit(f'--thresh {t!r}: the value is not finite')
    if not is_logit:
        if not 0.0 < x < 1.0:
            raise SystemExit(f'--thresh {t!r}: a probability lies strictly between 0 and 1 (a logit is given as logit:X)')
        x = math.log(x / (1.0 - x))
    with np.errstate(over='ignore'):
        v = float(np.float32(x))
    if not math.isfinite(v):
        raise SystemExit(f'--thresh {t!r}: the logit is not finite in fp32')
    return None if v == 0.0 else v


def thr_switches(args, mission=None):
    """(sweep, thresh) of --thr_sweep / --thresh (or the YAML keys `thr_sweep`, `thresh`): whether the validations sweep
    the threshold, and the fp32 logit every sigmoid decision is taken at (None: the default).  The missions and
    combinations they cannot serve and the values that are not understood are refused by name (SystemExit), host only."""
    mission = mission or getattr(args, 'mission', None)
    sweep = bool(getattr(args, 'thr_sweep', False))
    given = getattr(args, 'thresh', None)
    if sweep:
        if mission in ('prep', 'predict'):
            raise SystemExit(f'--thr_sweep sweeps the threshold of a validation against labels: the {mission} mission '
                             f'validates nothing, drop --thr_sweep')
        for switch in ('unlabelled', 'synthetic'):
            if getattr(args, switch, False):
                raise SystemExit(f'--thr_sweep --{switch}: the sweep counts labelled and unlabelled voxels, and there is '
                                 f'no truth: drop --thr_sweep')
        if getattr(args, 'no_test', False):
            raise SystemExit('--thr_sweep --no_test: the sweep belongs to the validation that --no_test skips: drop one '
                             'of them')
    thresh = None
    if given is not None:
        if mission == 'prep':
            raise SystemExit('--thresh sets the threshold of a decision: the prep mission decides nothing, drop --thresh')
        thresh = parse_thresh(given)
        if not getattr(args, 'multi_label', None):
            raise SystemExit(f'--thresh {given}: without --multi_label the classes are decided by argmax (class-id mode), '
                             f'which has no threshold: it needs --multi_label')
    return sweep, thresh


def match_switches(args, mission=None):
    """Whether --lesion_match (or the YAML key `lesion_match`) is set; the missions and combinations it cannot serve
    are refused by name (SystemExit), host only."""
    mission = mission or getattr(args, 'mission', None)
    if not getattr(args, 'lesion_match', False):
        return False
    if mission in ('prep', 'predict'):
        raise SystemExit(f'--lesion_match matches the lesions of a validation against labels: the {mission} mission '
                         f'validates nothing, drop --lesion_match')
    for switch in ('unlabelled', 'synthetic'):
        if getattr(args, switch, False):
            raise SystemExit(f'--lesion_match --{switch}: predicted lesions are matched to labelled ones, and there are '
                             f'no labels: drop --lesion_match')
    if getattr(args, 'no_test', False):
        raise SystemExit('--lesion_match --no_test: the matching belongs to the validation that --no_test skips: drop '
                         'one of them')
    return True


def prob_switches(args, mission=None):
    """(save_prob, save_unc) of --save_prob / --save_unc (or the YAML keys `save_prob`, `save_unc`); the missions that
    write no maps on a scan's grid refuse them by name (SystemExit), host only."""
    mission = mission or getattr(args, 'mission', None)
    got = tuple(bool(getattr(args, k, False)) for k in ('save_prob', 'save_unc'))
    for on, switch in zip(got, ('save_prob', 'save_unc')):
        if on and mission == 'prep':
            raise SystemExit(f'--{switch} writes the probabilities behind a predicted label map: the prep mission '
                             f'predicts nothing, drop --{switch}')
        if on and mission == 'ptq':
            raise SystemExit(f'--{switch} writes maps on the grid of a source scan: the ptq mission validates on the '
                             f'working grid (--save_nii writes its label maps), it belongs to the predict mission: drop '
                             f'--{switch}')
    return got


SCORE_MAX_CLASSES = 8        # effq_hip.h: EFFQ_SEG_TALLIES_MAX_CLASSES
SCORE_MAX_TOLS = 8           # effq_hip.h: EFFQ_SURF_TOL_MAX
SCORE_SWITCHES = ('pred_dir', 'score_class', 'score_tol')
# the label values of every class of a task's maps (brats: WT, TC, ET - evaluate.post_class_lut('brats', 3); lits: the
# liver with its tumours, the tumours)
SCORE_CLASSES = {'brats': ((1, 2, 4), (1, 4), (4,)), 'lits': ((1, 2), (2,))}
SCORE_TOL_DEFAULT = (1.0,)
# switches of the other missions that decide, clean or write maps: (name, the value that means "not given")
SCORE_FOREIGN = (('post', None), ('thresh', None), ('thr_sweep', False), ('save_prob', False), ('save_unc', False),
                 ('lesion_match', False), ('lesion_table', False), ('blend', 'uniform'), ('tta_mirror', None),
                 ('resume', None), ('pretrain', None), ('prep_mask', None), ('prep_window', None), ('prep_orient', None),
                 ('prep_spacing', None), ('prep_antialias', False), ('prep_interp', 'linear'), ('prep_min_size', None),
                 ('prep_no_crop', False))
# refused like those; kept apart because tests/test_score_cpu.py pins the members of SCORE_FOREIGN
SCORE_FOREIGN_ALIGN = (('prep_align', None),)


def parse_score_class(text) -> tuple:
    """The label values of one --score_class LABELS (a comma separated string, or a YAML list or integer); what is not
    understood is refused by name (SystemExit)."""
    parts = [str(v) for v in text] if isinstance(text, (list, tuple)) else str(text).split(',')
    labels = []
    for v in parts:
        if not re.fullmatch(r'\s*\d+\s*', v) or not 1 <= int(v) <= 255:
            raise SystemExit(f'--score_class {text!r}: label {v.strip()!r}: the label values of a class are 1 to 255')
        if int(v) in labels:
            raise SystemExit(f'--score_class {text!r}: label {int(v)} is given twice')
        labels.append(int(v))
    return tuple(labels)


def parse_score_tol(value) -> tuple:
    """The tolerances in mm of --score_tol T[,T...] (or a YAML number or list), sorted ascending; () for `none`.  What is
    not understood is refused by name (SystemExit)."""
    import math
    if value is None:
        return SCORE_TOL_DEFAULT
    if isinstance(value, str) and value.strip().lower() == 'none':
        return ()
    parts = list(value) if isinstance(value, (list, tuple)) else str(value).split(',')
    tols = []
    for v in parts:
        try:
            t = float(v)
        except (TypeError, ValueError):
            raise SystemExit(f'--score_tol {value!r}: {str(v).strip()!r} is no number: tolerances in mm, comma separated, '
                             f'or none')
        if not math.isfinite(t) or t < 0:
            raise SystemExit(f'--score_tol {value!r}: {str(v).strip()}: a tolerance is finite and >= 0 (millimetres)')
        if t in tols:
            raise SystemExit(f'--score_tol {value!r}: {t:g} is given twice')
        tols.append(t)
    if not 1 <= len(tols) <= SCORE_MAX_TOLS:
        raise SystemExit(f'--score_tol {value!r}: {len(tols)} tolerances, 1 to {SCORE_MAX_TOLS} (or none)')
    if len({'%g' % t for t in tols}) != len(tols):
        raise SystemExit(f'--score_tol {value!r}: two tolerances print alike (%g) and would share a column')
    return tuple(sorted(tols))


def score_class_lut(classes) -> list:
    """The 256-entry class table of effq_label_tallies for `classes`: bit c set = the value is one of classes[c]."""
    lut = [0] * 256
    for c, labels in enumerate(classes):
        for v in labels:
            lut[v] |= 1 << c
    return lut


def score_switches(args, mission=None):
    """(classes, tolerances) of --score_class / --score_tol (or the YAML keys `score_class`, a list, and `score_tol`) for
    the score mission: a tuple of label-value tuples (the task's default without the switch) and the tolerances in mm,
    ascending.  The other missions refuse --pred_dir, --score_class and --score_tol by name, and the score mission
    refuses every switch that decides, cleans or writes maps (SystemExit), host only."""
    mission = mission or getattr(args, 'mission', None)
    if mission != 'score':
        for switch in SCORE_SWITCHES:
            if getattr(args, switch, None) is not None:
                raise SystemExit(f'--{switch} belongs to the score mission, which scores finished maps against labels: '
                                 f'the {mission} mission scores nothing with it, drop --{switch}')
        return None
    for switch, unset in SCORE_FOREIGN + SCORE_FOREIGN_ALIGN:
        got = getattr(args, switch, unset)
        if got is not None and got != unset and got != []:
            raise SystemExit(f'--{switch} decides, cleans or writes maps: the score mission reads finished maps as they '
                             f'are (--pred_dir) and changes none, drop --{switch}')
    task = (getattr(args, 'task', None) or '').lower()
    given = getattr(args, 'score_class', None)
    if given is None or given == []:
        if task not in SCORE_CLASSES:
            raise SystemExit(f'score: --task {getattr(args, "task", None)!r}, one of {", ".join(SCORE_CLASSES)}')
        classes = SCORE_CLASSES[task]
    else:
        if isinstance(given, (str, int)):
            given = [given]
        if len(given) > SCORE_MAX_CLASSES:
            raise SystemExit(f'--score_class: {len(given)} classes, at most {SCORE_MAX_CLASSES}')
        classes = tuple(parse_score_class(t) for t in given)
    return classes, parse_score_tol(getattr(args, 'score_tol', None))


MEASURE_SWITCHES = ('lesion_measures', 'measure_class', 'measure_plane')
MEASURE_PLANES = ('axial', 'd', 'h', 'w')


def measure_switches(args, mission=None):
    """None without --lesion_measures, else (classes, plane) of --measure_class / --measure_plane (or the YAML keys
    `lesion_measures`, `measure_class`, a list, and `measure_plane`): a tuple of label-value tuples, or None for the
    mission's own classes (score: those of --score_class; predict: the task's), and one of MEASURE_PLANES.  ptq and prep
    refuse all three by name, score refuses --measure_class, and the two that only qualify the first are refused without
    it (SystemExit), host only."""
    mission = mission or getattr(args, 'mission', None)
    given = {k: getattr(args, k, None) for k in MEASURE_SWITCHES}
    given = {k: v for k, v in given.items() if v not in (None, False, [])}
    if mission in ('ptq', 'prep'):
        for switch in given:
            raise SystemExit(f'--{switch} measures the lesions of finished maps on the grid of their scan: the {mission} '
                             f'mission writes none, it belongs to the score and predict missions: drop --{switch}')
        return None
    if mission == 'score' and 'measure_class' in given:
        raise SystemExit('--measure_class: the score mission measures the classes it scores, those of --score_class: '
                         'drop --measure_class')
    if 'lesion_measures' not in given:
        for switch in given:
            raise SystemExit(f'--{switch} qualifies --lesion_measures, which is not given: add --lesion_measures or drop '
                             f'--{switch}')
        return None
    plane = given.get('measure_plane', 'axial')
    if plane not in MEASURE_PLANES:
        raise SystemExit(f'--measure_plane {plane!r}: one of {", ".join(MEASURE_PLANES)}')
    classes = given.get('measure_class')
    if classes is not None:
        if isinstance(classes, (str, int)):
            classes = [classes]
        if len(classes) > SCORE_MAX_CLASSES:
            raise SystemExit(f'--measure_class: {len(classes)} classes, at most {SCORE_MAX_CLASSES}')
        try:
            classes = tuple(parse_score_class(t) for t in classes)
        except SystemExit as e:
            raise SystemExit(str(e).replace('--score_class', '--measure_class'))
    return classes, plane


POST_MAX_RULES = 8           # effq_hip.h: EFFQ_LABEL_CLEAN_MAX_RULES
POST_MAX_RADIUS = 32         # effq_hip.h: EFFQ_LABEL_POST_MAX_RADIUS
POST_CONN_DEFAULT = 26       # the neighbourhood of --is_cc
# labels: tuple of 1..255; op: largest / min (n voxels) / fill / close / open (n = the radius R in voxels)
PostRule = collections.namedtuple('PostRule', 'labels op n to')
POST_GROWING_OPS = ('fill', 'close')         # they add voxels to the mask: TO is one of LABELS


def post_rule_text(rule) -> str:
    """A rule in the form --post takes it: `1,2:largest`, `4:min500>1`, `1,2:fill>1`, `1:close2>1`, `2:open3`."""
    labels, op, n, to = rule
    said = ','.join(str(v) for v in labels) + ':' + op + (str(n) if op in ('min', 'close', 'open') else '')
    return said + (f'>{to}' if to or op in POST_GROWING_OPS else '')


def post_text(rules, connectivity=POST_CONN_DEFAULT) -> str:
    """The `post` column of predict.csv: the rules joined by a space, ` conn6` when the neighbourhood is not the default."""
    return ' '.join([post_rule_text(r) for r in rules] +
                    ([f'conn{connectivity}'] if connectivity != POST_CONN_DEFAULT else []))


def parse_post_rule(text) -> PostRule:
    """One RULE = LABELS ":" OP [ ">" TO ] of --post; what is not understood is refused by name (SystemExit)."""
    t = str(text).strip()
    m = re.fullmatch(r'([^:>]*):([^:>]*)(?:>([^:>]*))?', t)
    if m is None:
        raise SystemExit(f'--post {t!r}: a rule is LABELS:OP or LABELS:OP>TO, as in 1,2:largest or 4:min500>1')
    labs, op, to = m.group(1).strip(), m.group(2).strip(), m.group(3)
    if not labs:
        raise SystemExit(f'--post {t!r}: empty LABELS: name the label values of the mask, as in 1,2:largest')
    labels = []
    for v in labs.split(','):
        if not re.fullmatch(r'\s*\d+\s*', v) or not 1 <= int(v) <= 255:
            raise SystemExit(f'--post {t!r}: label {v.strip()!r}: the label values of a mask are 1 to 255')
        if int(v) not in labels:
            labels.append(int(v))
    mm = re.fullmatch(r'(min|close|open)\s*(-?\d+)', op)
    if op in ('largest', 'fill'):
        name, n = op, 0
    elif mm is not None:
        name, n = mm.group(1), int(mm.group(2))
        if name == 'min' and n < 1:
            raise SystemExit(f'--post {t!r}: min {n}: N is a size in voxels, 1 or more')
        if name != 'min' and not 1 <= n <= POST_MAX_RADIUS:
            raise SystemExit(f'--post {t!r}: {name} {n}: R is a radius in voxels, 1 to {POST_MAX_RADIUS}')
    else:
        raise SystemExit(f'--post {t!r}: unknown op {op!r}: one of largest, minN (N voxels), fill, closeR, openR '
                         f'(R voxels)')
    grows = name in POST_GROWING_OPS
    dest = labels[0] if grows else 0
    if to is not None:
        if not re.fullmatch(r'\s*\d+\s*', to) or int(to) > 255:
            raise SystemExit(f'--post {t!r}: TO {to.strip()!r}: the new label is 0 to 255')
        dest = int(to)
    if grows and dest not in labels:
        raise SystemExit(f'--post {t!r}: TO {dest} is not one of LABELS: {name} adds voxels to the mask, so they take '
                         f'one of its labels')
    if not grows and dest in labels:
        raise SystemExit(f'--post {t!r}: TO {dest} is one of LABELS: the relabelled voxels would stay in the mask')
    return PostRule(tuple(labels), name, n, dest)


def parse_post_text(text):
    """(rules, connectivity) back from post_text's string."""
    words = str(text).split()
    conn = POST_CONN_DEFAULT
    if words and words[-1].startswith('conn'):
        conn = int(words.pop()[4:])
    return [parse_post_rule(w) for w in words], conn


def post_rules(args):
    """(rules, connectivity) of --post / --post_conn (or the YAML keys `post`, a list, and `post_conn`): a list of PostRule
    in the order given ([] without --post) and 6 or 26.  What is not understood is refused by name (SystemExit), host
    only."""
    given = getattr(args, 'post', None)
    conn = getattr(args, 'post_conn', None)
    if given is None or given == []:
        if conn is not None:
            raise SystemExit(f'--post_conn {conn}: the neighbourhood of the --post rules, and no --post is given')
        return [], POST_CONN_DEFAULT
    if isinstance(given, (str, int)):
        given = [given]
    if len(given) > POST_MAX_RULES:
        raise SystemExit(f'--post: {len(given)} rules, at most {POST_MAX_RULES}')
    rules = [parse_post_rule(t) for t in given]
    if conn is None:
        return rules, POST_CONN_DEFAULT
    if str(conn).strip() not in ('6', '26'):
        raise SystemExit(f'--post_conn {conn!r}: one of 6, 26')
    return rules, int(conn)


def _pair(s):
    return [int(x) for x in s.split(',')] if s else None


def get_conv_class(args):
    """(QConv class, Qinfo string naming the snapshot dir, kwQ) -- definer.py:286-329."""
    name = args.qconv.lower()
    if name not in QCONV_REGISTRY:
        raise RuntimeError('Unknown QConv name: %s' % args.qconv)
    if name == 'conv':
        return nn.Conv3d, 'FP', {}
    q_weight, q_act = args.qlvl_w > 0, args.qlvl_a > 0
    qlvl, qlvl_act = args.qlvl_w, (args.qlvl_a if q_act else 256)
    kwQ = {a: getattr(args, a) for a in dir(args) if a[:4] == 'lwq_'}
    if q_act and q_weight:
        info = 'bothQw{}a{}'.format(qlvl, qlvl_act)
    elif q_act:
        info = 'actQa{}'.format(qlvl_act)
    else:
        info = 'weightQw{}'.format(qlvl)
    return QCONV_REGISTRY[name], args.qconv + '_' + info, kwQ


def get_model_cube(args, QConv=nn.Conv3d, kwQ=None):
    """definer.py:130-248."""
    kwQ = kwQ or {}
    task = args.task.lower()
    nMod = args.nMod if args.nMod else (4 if task == 'brats' else 1)
    nClass = args.nClass if args.nClass else (4 if task == 'brats' else 3)
    if getattr(args, 'bin_label', None):
        nClass = 2
    if getattr(args, 'multi_label', None):
        nClass -= 1
    if args.model not in ('UResQ',):
        raise RuntimeError('Unknown model name: %s' % args.model)
    st = str(args.init_stride)
    init_stride = tuple(int(x) for x in st.split(',')) if ',' in st else (int(st),) * 3
    if args.qconv.lower() == 'conv':
        q_weight = q_act = False
        q_first = q_last = qlvl = qlvl_act = None
    else:
        q_weight, q_act = args.qlvl_w > 0, args.qlvl_a > 0
        qlvl, qlvl_act = args.qlvl_w, (args.qlvl_a if q_act else 256)
        q_first, q_last = _pair(args.q_first), _pair(args.q_last)
    if args.nla.lower() not in ('relu', 'reluf'):
        raise RuntimeError('Unknown NLA name: %s' % args.nla)
    if args.norm.lower() != 'bn':
        raise NotImplementedError('Norm type should be in BN')
    width = [int(i) for i in args.width.split(',')] if args.width else [32, 64, 128, 256, 128, 64, 32]
    depth = [int(i) for i in args.depth.split(',')] if args.depth else [1] * len(width)
    dil = [int(i) for i in args.dilation.split(',')] if args.dilation else [1] * len(width)
    hp = {'drop_cut_thres': 128, 'ds_depth_limit': 3 if 2 in init_stride else 4}
    if args.hetero_dim:
        hp['aniso_pool_depth'] = 9999 if 2 in init_stride else 4
        hp['aniso_pool_stride'] = (2, 2, 1)
    model = UResQ(QConv, nMod, nClass, depth_config=depth, width_config=width, dilation_config=dil,
                  init_stride=init_stride, stride=2, drop_rate=args.drop_rate, bn=nn.BatchNorm3d, ds=args.ds,
                  blk_type=args.blk, q_weight=q_weight, qlvl=qlvl, q_act=q_act, qlvl_act=qlvl_act,
                  q_first=q_first, q_last=q_last, hetero_param=hp, init_kernel=args.init_kernel, **kwQ)
    num_mo = min(hp['ds_depth_limit'], len(depth) // 2 + 1) if args.ds else 1
    cube = {'model': model, 'init_func': None, 'pretrain': args.pretrain, 'resume': getattr(args, 'resume', None),
            'optimizer_list': None, 'num_mo': num_mo, 'nClass': nClass, 'nMod': nMod}
    return cube, args.model + '_' + args.norm.upper()


BRATS_NET = dict(task='brats', model='UResQ', nMod=4, nClass=4, multi_label='brats', init_stride='2,2,2',
                 depth='1,1,1,1,1,1,1', width='32,64,128,256,128,64,32', dilation='1,1,1,1,1,1,1', nla='relu',
                 norm='bn', drop_rate=0.5, ds='simple', hetero_dim=True, blk='mid', init_kernel=3,
                 qconv='effq', q_first='256,-1', q_last='256,-1')       # config/brats_ptq.yaml
LITS_NET = dict(task='lits', model='UResQ', nMod=1, nClass=3, multi_label=None, init_stride='2,2,1',
                depth='1,1,1,1,1,1,1,1,1', width='32,64,128,256,512,256,128,64,32',
                dilation='1,1,1,1,1,1,1,1,1', nla='relu', norm='bn', drop_rate=0.5, ds='simple', hetero_dim=True,
                blk='mid', init_kernel=3, qconv='effq', q_first='256,-1', q_last='256,-1')   # config/lits_ptq.yaml
TINY_NET = dict(task='lits', model='UResQ', nMod=1, nClass=3, multi_label=None, init_stride='1', depth='1,1,1',
                width='8,16,8', dilation=None, nla='relu', norm='bn', drop_rate=0.5, ds='simple', hetero_dim=True,
                blk='mid', init_kernel=3, qconv='effq', q_first='256,-1', q_last='256,-1')   # BASELINE config 1


def make_args(net: dict, qlvl_w: int, qlvl_a: int, **over):
    base = dict(pretrain=None, resume=None, device=0, round='1', suffix='', config=None, test_fp=False,
                no_test=True, save_nii=False, is_cc=False, surf_dist=False, lesion_table=False, lesion_match=False, vs_fp=False, unlabelled=False, src_geom=False, spacing=None, post=None, post_conn=None, bin_label=None, lwq_dataid=0, lwq_batchsz=1, lwq_patchsz=None,
                lwq_verbose=False, qlvl_w=qlvl_w, qlvl_a=qlvl_a)
    base.update(net)
    base.update(over)
    return argparse.Namespace(**base)
