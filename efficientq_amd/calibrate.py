"""PTQ orchestrator with the reference's ``do_ptq`` contract (src/ptqer.py:282-387): FP pass with
per-layer target capture, attention-mask pyramid, one quantising pass in network order, timing
(t2 - t0), ``layer_loss.txt`` / ``time_cost.txt`` / ``class_voxel_nums.txt`` and the three
snapshots.  Differences, all deliberate and MI355X-first:
  * FP targets and masks stay in HBM (the reference parks them on the host, hooks.py:6);
  * with ``torch.distributed`` initialised, ``data_batch`` is this rank's shard of the calibration
    volumes and every volume-summed statistic is all-reduced (RCCL), see qconv.SumReducer;
  * the Qseg / FPseg NIfTI maps of the calibration volumes are written with ``--save_nii`` only, by the HIP label
    kernel and the nibabel-free writer of nifti.py.
"""
from __future__ import annotations

import copy
import os
import os.path as P
import time
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .qconv import PTQConv, SumReducer


# ---- mode / attribute broadcasters (ptqer.py:17-80) ----------------------------------------------
def _each_q(m: nn.Module):
    for name, mod in m.named_modules():
        if isinstance(mod, PTQConv):
            yield name, mod


def set_fp(m):
    for _, q in _each_q(m):
        q.set_fp()


def set_quantizing(m):
    for _, q in _each_q(m):
        q.set_quantizing()


def set_quantized(m):
    for _, q in _each_q(m):
        q.set_quantized()


def set_init_alpha(m):
    for _, q in _each_q(m):
        q.set_init_act()


def store_int_weight(m):
    for _, q in _each_q(m):
        q.store_int_weight()


def restore_fp_weight(m):
    for _, q in _each_q(m):
        q.restore_fp_weight()


def set_anything(m, attr, value):
    for _, q in _each_q(m):
        setattr(q, attr, value)


def set_name(m):
    for name, q in _each_q(m):
        q.name = name


def set_snapdir(m, snap_dir):
    set_anything(m, 'snap_dir', snap_dir)


def set_mask(m, pyramid):
    set_anything(m, 'mask_pyramid', pyramid)


def set_debug(m):
    set_anything(m, 'debug', True)


# ---- BN folding (fold_bn.py:14-46,68-80) -----------------------------------------------------------
class StraightThrough(nn.Module):
    def forward(self, x):
        return x


def _absorbs(m):
    return isinstance(m, (nn.Conv2d, nn.Conv3d, nn.Linear))


def _is_bn(m):
    return isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d))


def fold_bn_pair(conv: nn.Module, bn: nn.Module):
    """W' = W*gamma/sqrt(var+eps), b' = beta - gamma*mean/sqrt(var+eps) (+ gamma*b/sqrt(..))."""
    w = conv.weight.data
    sd = torch.sqrt(bn.running_var + bn.eps)
    shape = (conv.out_channels,) + (1,) * (w.dim() - 1)
    if bn.affine:
        w2 = w * (bn.weight / sd).view(shape)
        shift = bn.bias - bn.weight * bn.running_mean / sd
        b2 = bn.weight * conv.bias / sd + shift if conv.bias is not None else shift
    else:
        w2 = w / sd.view(shape)
        shift = -bn.running_mean / sd
        b2 = conv.bias / sd + shift if conv.bias is not None else shift
    if conv.bias is None:
        conv.bias = nn.Parameter(b2.detach().clone())
    else:
        conv.bias.data = b2.detach()
    conv.weight.data = w2.detach()


def search_fold_and_remove_bn(model: nn.Module):
    """Fold every eval-mode BN that directly follows a conv (in child order) and replace it by an
    identity; returns the last absorbing module seen, exactly like the reference's recursion."""
    model.eval()
    prev = None
    for name, child in model.named_children():
        if _is_bn(child) and _absorbs(prev):
            fold_bn_pair(prev, child)
            setattr(model, name, StraightThrough())
        elif _absorbs(child):
            prev = child
        else:
            prev = search_fold_and_remove_bn(child)
    return prev


# ---- predictions and attention masks (metrics.py:172-192, ptqer.py:141-235) --------------------------
def get_pred_lits(out):
    return torch.max(out, 1)[1]


def get_pred_brats(out):
    hard = torch.sigmoid(out) >= 0.5
    pred = torch.zeros_like(hard[:, 0]).int()
    for c in range(hard.shape[1]):
        pred[hard[:, c]] = c + 1          # last positive channel wins (quirk Q3)
    return pred


def _stride3(init_stride):
    if isinstance(init_stride, str):
        return tuple(int(v) for v in init_stride.split(',')) if ',' in init_stride else (int(init_stride),) * 3
    return tuple(init_stride) if isinstance(init_stride, (tuple, list)) else (int(init_stride),) * 3


def get_att_weight_map(output_fp, body_mask, style: str, task: str = 'lits', reducer=None):
    """Class census over ALL calibration volumes and w_c = (max n / n_c)^p (ptqer.py:209-235)."""
    out = output_fp[-1]
    if task == 'lits':
        pred = torch.max(out, 1)[1]
        counts = torch.stack([((pred == c) & body_mask).sum() for c in range(3)])
    elif task == 'brats':
        hard = (torch.sigmoid(out) >= 0.5).int()
        bkg = (hard.sum(dim=1) == 0).sum() - (~body_mask).sum()
        counts = torch.stack([bkg] + [(hard[:, c] * body_mask).sum() for c in range(3)])
    else:
        raise RuntimeError(f'Unknown task {task}')
    counts = counts.to(torch.int64)
    if reducer is not None:
        reducer(counts)
    nums = counts.tolist()
    if 'p:' not in style:
        raise RuntimeError(f'Unknown attention weight map style {style}')
    p = float(style[2:])
    wmap = {c: (1.0 if n == 0 else (1 / n * max(nums)) ** p) for c, n in enumerate(nums)}
    return wmap, nums


def get_mask_pyramid(output_fp, body_mask, weight_map: dict, init_stride, num_lvls: int = 5, task='lits'):
    """ptqer.py:141-167.  The mask inherits the prediction's INTEGER dtype, so the float weights are
    truncated toward zero on assignment (quirk Q1); non-body voxels are reset to 1."""
    st = _stride3(init_stride)
    out = F.avg_pool3d(output_fp[-1], st)
    body = F.max_pool3d(body_mask.float(), st).bool()
    pyramid = []
    for _ in range(num_lvls):
        pred = get_pred_lits(out) if task == 'lits' else get_pred_brats(out)
        if task not in ('lits', 'brats'):
            raise RuntimeError(f'Unknown task {task}')
        mask = torch.ones_like(pred)
        for cls, wv in weight_map.items():
            mask[pred == cls] = wv
        mask[~body] = 1
        pyramid.append(mask.float())
        if min(out.shape[2:]) < 2:
            break
        out = F.avg_pool3d(out, 2)
        body = F.max_pool3d(body.float(), 2).bool()
    return pyramid


# ---- calibration data (ptqer.py:83-111) -----------------------------------------------------------
def center_crop(t: torch.Tensor, size):
    """Centre crop of the last three dims, zero-padding first when smaller (dataloader/transforms.py:60-93)."""
    for ax, target in zip((-1, -2, -3), (size[2], size[1], size[0])):
        cur = t.shape[ax]
        if cur < target:
            lo = (target - cur) // 2
            pad = [0, 0] * 3
            pad[2 * (-ax - 1)], pad[2 * (-ax - 1) + 1] = lo, target - cur - lo
            t = F.pad(t, pad)
    d, h, w = t.shape[-3:]
    x1, y1, z1 = (d - size[0]) // 2, (h - size[1]) // 2, (w - size[2]) // 2
    return t[..., x1:x1 + size[0], y1:y1 + size[1], z1:z1 + size[2]]


def _crop_label(label, crop):
    """The label cropped like its image; an unlabelled volume's empty label (--unlabelled) stays as it is."""
    return label if label.numel() == 0 else center_crop(label, crop)


def get_calibration_data(args, data_cube):
    data_cube.trainseqloader.dataset.use_fix_transform()
    it = iter(data_cube.trainseqloader)
    for _ in range(args.lwq_dataid):
        next(it)
    if args.lwq_batchsz == 1:
        data, label = next(it)
        crop = [int(v) for v in args.lwq_patchsz.split(',')] if args.lwq_patchsz else \
            [min(v, 192) // 64 * 64 for v in data.shape[-3:]]
        return center_crop(data, crop), _crop_label(label, crop)
    crop = [int(v) for v in args.lwq_patchsz.split(',')]
    ds, ls = [], []
    for _ in range(args.lwq_batchsz):
        d, l = next(it)
        ds.append(center_crop(d, crop))
        ls.append(_crop_label(l, crop))
    return torch.cat(ds, 0), torch.cat(ls, 0)


# ---- the calibration run ---------------------------------------------------------------------------
# hooks.py:5-6 stores `o.detach().cpu()`.  With the model on a GPU - the reference's intended device - that is a COPY,
# taken before the next block's in-place ReLU (factoryQ.py:76-77) rewrites the conv's output.  With the model on the CPU
# `.cpu()` returns the tensor itself, and the targets of the 11 convs (of 22, BraTS net) that feed an in-place ReLU
# silently become relu(y): the reference then calibrates those layers against the wrong target (first-layer loss 0.125
# instead of 1.3e-4 on the BraTS net, FP-vs-Q agreement 0.93 instead of 0.99).  Default here: the copy (GPU behaviour);
# ALIAS_FP_TARGETS / EFFQ_ALIAS_FP_TARGETS=1 reproduces a CPU run of the reference (what the g6 fixtures hold).
import os as _os
ALIAS_FP_TARGETS = _os.environ.get("EFFQ_ALIAS_FP_TARGETS", "0") == "1"


def forward_hook(m, i, o):
    """FP target capture; stays on the device."""
    m.output_fp = o.detach() if ALIAS_FP_TARGETS else o.detach().clone()


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize(device)


def calibrate_model(model: nn.Module, data_batch: torch.Tensor, task: str, init_stride, verbose=False):
    """The timed window of do_ptq (ptqer.py:313-364).  Returns a dict with output_fp, output_q,
    layer_loss (list of str), class nums, mask pyramid and the three time stamps."""
    device = data_batch.device
    red = SumReducer()
    handles = []

    def reg(mod):
        if isinstance(mod, PTQConv):
            handles.append(mod.register_forward_hook(forward_hook))
        else:
            for c in mod.children():
                reg(c)
    reg(model)
    model.eval()
    _sync(device)
    t0 = time.time()
    set_fp(model)
    with torch.no_grad():
        output_fp = model(data_batch).detach()
        ones = torch.ones_like(data_batch[:, 0]).bool()
        body = (data_batch[:, 0] != 0.0).bool() if task == 'brats' else ones
        wmap, nums = get_att_weight_map(output_fp, ones, 'p:0.5', task=task, reducer=red or None)   # quirk Q2
        pyramid = get_mask_pyramid(output_fp, body, wmap, init_stride, num_lvls=5, task=task)
    set_mask(model, pyramid)
    for h in handles:
        h.remove()
    layer_loss: List[str] = []
    set_anything(model, 'layer_loss', layer_loss)
    set_anything(model, 'lwq_verbose', verbose)
    _sync(device)
    t1 = time.time()
    set_quantizing(model)
    with torch.no_grad():
        output_q = model(data_batch)
    _sync(device)
    t2 = time.time()
    set_quantized(model)
    return dict(output_fp=output_fp, output_q=output_q, layer_loss=layer_loss, nums=nums, pyramid=pyramid,
                weight_map=wmap, t0=t0, t1=t1, t2=t2)


def do_ptq(args, model_cube, data_cube, tester, snap_dir):
    model = model_cube['model']
    pretrain = model_cube['pretrain']
    device = torch.device(args.device if not isinstance(args.device, int) else f'cuda:{args.device}')
    print('pretrain is :', pretrain)
    sd = torch.load(pretrain, map_location='cpu')['state_dict']
    model.load_state_dict(sd, strict=False)
    model.eval()
    search_fold_and_remove_bn(model)
    model.to(device)
    # --vs_fp: the network as it is before the calibration rewrites its weights, to validate the calibrated one against
    fp_model = None
    if getattr(args, 'vs_fp', False) and not args.no_test:
        fp_model = copy.deepcopy(model)
        fp_model.eval()
        set_fp(fp_model)

    data_batch, label_batch = get_calibration_data(args, data_cube)
    data_batch = data_batch.to(device)
    set_name(model)
    set_snapdir(model, snap_dir)
    set_fp(model)
    # the lesion and surface switches are passed only when they are set: a tester that knows (folder, is_save_nii)
    # alone keeps working
    cc = {'is_cc': True} if getattr(args, 'is_cc', False) else {}
    if getattr(args, 'surf_dist', False):
        cc['is_surf'] = True
    if getattr(args, 'lesion_table', False):
        cc['is_table'] = True
    if getattr(args, 'lesion_match', False):
        cc['is_match'] = True
    if args.test_fp:
        tester.test_as_is(folder='fp', is_save_nii=args.save_nii, **cc)

    res = calibrate_model(model, data_batch, args.task, args.init_stride, verbose=bool(args.lwq_verbose))
    body = (data_batch[:, 0] != 0.0) if args.task == 'brats' else torch.ones_like(data_batch[:, 0]).bool()
    print(f'Body occupies {body.sum() / body.numel() * 100}% of the volume.')
    t0, t1, t2 = res['t0'], res['t1'], res['t2']
    print(f'FP forward costs {t1 - t0:.3f}s, PTQ costs {t2 - t1:.3f}s, totally {t2 - t0:.3f}s.')
    os.makedirs(snap_dir, exist_ok=True)
    with open(P.join(snap_dir, 'class_voxel_nums.txt'), 'w') as fid:
        for n in res['nums']:
            fid.write(f'{n}\n')
    with open(P.join(snap_dir, 'time_cost.txt'), 'w') as fid:
        fid.write(f'{(t2 - t0) / 60:.3f} min.')
    with open(P.join(snap_dir, 'layer_loss.txt'), 'w') as fid:
        fid.write('\n'.join(res['layer_loss']))
    if args.save_nii:
        _save_nifti(res, args.task, snap_dir)

    if not args.no_test:
        if fp_model is not None:        # passed only when set: a tester that does not know the keyword keeps working
            cc['fp_model'] = fp_model
        tester.test_as_is('ptq', args.save_nii, **cc)
    fp_model = None
    model.cpu()
    tester.snapshot('state_in_fp.pkl', compress=False)
    store_int_weight(model)
    tester.snapshot('state_in_int8.pkl', compress=False)
    tester.snapshot('state_in_int8_compress.npz', compress=True)
    return res


def load_calibrated(model: nn.Module, path: str, device):
    """Put a snapshot do_ptq wrote back into the freshly built `model` (the network of the same --config and levels):
    fold the BN layers as do_ptq does before it calibrates (the snapshots hold the folded network), load the state
    dict strictly, move the model to `device` and set it to the quantised mode.  Returns the model.
    state_in_fp.pkl: the weights as they are - the logits are those of the calibrated model in memory, bit for bit.
    state_in_int8.pkl (integer weights on the quantised convs): the level ids are loaded and every conv's
    restore_fp_weight() puts them back on alpha_w's grid.  In channel mode (alpha_w of shape (c2, 1, 1, 1): the model
    must be built with lwq_channel_wise) that is exact.  In per-tensor mode the snapshot holds the LAST iterate's alpha_w
    beside the BEST iterate's ids (quirk Q6): the restored weights lie on that grid but are not the calibrated weights;
    one line says so.
    A snapshot whose keys or shapes do not fit the network ends with a SystemExit naming the first missing and the
    first unexpected key; the model is then as it was built, but for the folding."""
    try:
        blob = torch.load(path, map_location='cpu')
    except Exception as e:
        raise SystemExit(f'--resume {path}: cannot read the snapshot: {e}')
    sd = blob.get('state_dict') if isinstance(blob, dict) else None
    if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
        raise SystemExit(f"--resume {path}: no 'state_dict' of tensors inside: not a snapshot of the ptq mission")
    model.eval()
    search_fold_and_remove_bn(model)
    own = model.state_dict()
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    shapes = [k for k in own if k in sd and tuple(own[k].shape) != tuple(sd[k].shape)]
    if missing or unexpected or shapes:
        parts = []
        if missing:
            parts.append(f'{len(missing)} keys of the network are missing, the first {missing[0]}')
        if unexpected:
            parts.append(f'{len(unexpected)} keys are unexpected, the first {unexpected[0]}')
        if shapes:
            k = shapes[0]
            parts.append(f'{len(shapes)} shapes differ, the first {k}: {tuple(sd[k].shape)} in the snapshot, '
                         f'{tuple(own[k].shape)} in the network')
        raise SystemExit(f'--resume {path}: the snapshot does not fit the network of --config (widths, levels, '
                         f'--lwq_channel_wise?): ' + '; '.join(parts))
    convs = list(_each_q(model))
    ints = [name for name, _ in convs if not sd[name + '.weight'].dtype.is_floating_point]
    if ints and len(ints) != len(convs):
        raise SystemExit(f'--resume {path}: integer weights on {len(ints)} of {len(convs)} quantised convs: the first '
                         f'is {ints[0]}')
    model.load_state_dict(sd, strict=True)
    if ints:
        restore_fp_weight(model)
        if not all(q.channel_wise for _, q in convs):
            print(f'[resume] {path}: per-tensor level ids were stored beside the last iterate\'s alpha_w, not the best '
                  f'iterate\'s (quirk Q6): the restored weights lie on that grid but are not the calibrated weights; '
                  f'state_in_fp.pkl holds those exactly')
    model.to(device)
    set_quantized(model)
    return model


def _volume_offset(n: int) -> int:
    """Index of this rank's first calibration volume in the whole batch: the volume count of the lower ranks."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return 0
    sizes = [None] * dist.get_world_size()
    dist.all_gather_object(sizes, int(n))
    return sum(sizes[:dist.get_rank()])


def _save_nifti(res, task, snap_dir):
    """Qseg{i}.nii.gz / FPseg{i}.nii.gz of the calibration volumes (ptqer.py:372-377, metrics.extract_nii): the last
    head's class ids for lits, get_pred_brats_con_merge for brats (effq_seg_labels), uint8 with the identity affine.
    i is the volume's index in the whole calibration batch, so data-parallel ranks write different files."""
    from .hip_ops import get_ops
    from .nifti import write_nifti
    if task not in ('lits', 'brats'):
        raise RuntimeError(f'Unknown task {task}')
    rule, fuse = ('argmax', None) if task == 'lits' else ('rank', 'con')
    first = None
    for tag, out in (('Qseg', res['output_q']), ('FPseg', res['output_fp'])):
        head = out[-1]
        maps = get_ops(head.device).seg_labels(head, rule, fuse).cpu().numpy()
        if first is None:
            first = _volume_offset(len(maps))
        for i, m in enumerate(maps):
            write_nifti(P.join(snap_dir, f'{tag}{first + i}.nii.gz'), m)
