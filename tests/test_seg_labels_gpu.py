"""Label maps on a real MI355X (-m gpu): effq_seg_labels bit for bit against torch restatements of the reference's
get_pred_lits, get_pred_brats_con_merge, merge_label_brats(merge_label_basic(...)) and merge_label_basic, its argument
checks, and the ptq mission's --save_nii output tied back to the tallies in metrics.csv."""
import csv
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.nifti import read_nifti
from tests.test_seg_eval_cpu import write_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


# ---- torch restatements (on the device) --------------------------------------------------------------------------
def merge_basic(hard, fuse):
    """misc.merge_label_basic over the channel axis (1) of N x C x ... 0/1 ints."""
    hard = hard.clone()
    if fuse in ("agg", "aggressive"):
        for i in range(hard.shape[1]):
            hard[:, i] = hard[:, i:].sum(1) > 0
    elif fuse in ("con", "conservative"):
        for i in range(1, hard.shape[1]):
            hard[:, i] = hard[:, i] * hard[:, i - 1]
    return hard


def pred_lits(x):
    """metrics.get_pred_lits."""
    return torch.max(x, 1)[1]


def pred_rank(x, fuse):
    """metrics.get_pred_brats_con_merge for fuse 'con' (get_pred_brats for None): i + 1 of the last set channel."""
    hard = merge_basic((torch.sigmoid(x) >= 0.5).int(), fuse)
    pred = torch.zeros_like(hard[:, 0])
    for i in range(hard.shape[1]):
        pred[hard[:, i] > 0] = i + 1
    return pred


def pred_brats(x, fuse):
    """misc.merge_label_brats(misc.merge_label_basic(...)) per case."""
    hard = merge_basic((torch.sigmoid(x) >= 0.5).int(), fuse)
    merged = torch.zeros_like(hard[:, 0])
    merged[hard[:, 0] != 0] = 1
    merged[(hard[:, 0] != 0) & (hard[:, 1] == 0)] = 2
    merged[hard[:, 2] != 0] = 4
    return merged


def pred_planes(x, fuse):
    return merge_basic((torch.sigmoid(x) >= 0.5).int(), fuse)


def _logits(ops, N, C, shape, seed, sigmoid):
    g = torch.Generator().manual_seed(seed)
    if not sigmoid:
        x = torch.randint(-2, 3, (N, C) + shape, generator=g).float()         # many exact ties
        nan = torch.rand((N,) + shape, generator=g) < 0.05
        ch = torch.randint(0, C, (N,) + shape, generator=g)
        n, d, h, w = nan.nonzero(as_tuple=True)
        x[n, ch[nan], d, h, w] = float("nan")                                   # one NaN in a voxel at most
        return x.to(DEV)
    x = torch.randn((N, C) + shape, generator=g)
    near = torch.rand(x.shape, generator=g) < 0.3
    x[near] = (torch.rand(int(near.sum()), generator=g) * 2 - 1) * 1e-8
    # the bisected threshold and up to 1024 ulps either side of it, spread over every channel and case
    t = ops.sigmoid_threshold()
    tb = int(torch.tensor([-t]).view(torch.int32))
    sweep = -torch.arange(tb - 1024, tb + 1024, dtype=torch.int32).view(torch.float32)
    flat = x.view(-1)
    k = min(sweep.numel(), flat.numel() // 2)
    flat[torch.randperm(flat.numel(), generator=g)[:k]] = sweep[:k]
    flat[:3] = torch.tensor([t, np.nextafter(np.float32(t), np.float32(-1)), np.nextafter(np.float32(t), np.float32(1))])
    return x.to(DEV)


SHAPES = [(7, 9, 11), (6, 10, 12)]      # 693 voxels (scalar path) and 720 (16-byte loads)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_argmax_equals_get_pred_lits(ops, C, N, shape, dtype):
    x = _logits(ops, N, C, shape, 10 * C + N, sigmoid=False)
    got = ops.seg_labels(x, "argmax", None, dtype)
    assert got.dtype == dtype and got.shape == (N,) + shape
    assert torch.equal(got.long(), pred_lits(x))


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_sigmoid_rules_equal_the_reference_merges(ops, C, N, shape, fuse):
    x = _logits(ops, N, C, shape, 100 * C + 10 * N + len(fuse or ""), sigmoid=True)
    for dtype in (torch.uint8, torch.uint16):
        got = ops.seg_labels(x, "rank", fuse, dtype)
        assert got.dtype == dtype and got.shape == (N,) + shape
        assert torch.equal(got.long(), pred_rank(x, fuse).long())
        if C >= 3:
            got = ops.seg_labels(x, "brats", fuse, dtype)
            assert torch.equal(got.long(), pred_brats(x, fuse).long())
    got = ops.seg_labels(x, "planes", fuse)
    assert got.dtype == torch.uint8 and got.shape == x.shape
    assert torch.equal(got.long(), pred_planes(x, fuse).long())


def test_grid_stride_and_unaligned_logits(ops):
    """More voxels than one pass of the capped grid covers, and logits off a 16-byte boundary (scalar path)."""
    x = _logits(ops, 1, 3, (130, 128, 128), 7, sigmoid=True)
    assert torch.equal(ops.seg_labels(x, "brats", "agg", torch.uint16).long(), pred_brats(x, "agg").long())
    assert torch.equal(ops.seg_labels(x, "argmax").long(), pred_lits(x))
    buf = torch.empty(1 + x.numel(), device=DEV)
    y = buf[1:].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 != 0
    assert torch.equal(ops.seg_labels(y, "rank", "con").long(), pred_rank(x, "con").long())


def test_argument_errors_raise_before_a_launch(ops):
    x = torch.zeros(1, 3, 4, 4, 4, device=DEV)
    bad = [
        (torch.zeros(1, 9, 4, 4, 4, device=DEV), "argmax", None, torch.uint8),      # too many classes
        (torch.zeros(3, 4, device=DEV)[0], "argmax", None, torch.uint8),            # no class axis
        (torch.zeros(1, 3, 4, 4, 4, device=DEV, dtype=torch.float64), "argmax", None, torch.uint8),
        (torch.zeros(1, 3, 4, 4, 4), "argmax", None, torch.uint8),                  # host tensor
        (x, "argmax", "agg", torch.uint8),                                          # argmax takes no merge
        (x, "planes", None, torch.uint16),                                          # planes are uint8
        (x, "rank", None, torch.int32),
        (x, "rank", "mean", torch.uint8),
        (x, "labels", None, torch.uint8),
        (x[:, :2], "brats", "agg", torch.uint8),                                    # brats needs 3 channels
        (torch.zeros(0, 3, 4, 4, 4, device=DEV), "rank", None, torch.uint8),
    ]
    for args in bad:
        with pytest.raises(_lib.EffqError):
            ops.seg_labels(*args)


# ---- the ptq mission with --save_nii ------------------------------------------------------------------------------
def _counts(pred, gt):
    return [int((pred & gt).sum()), int((pred & ~gt).sum()), int((~pred & gt).sum()), int((~pred & ~gt).sum())]


def _run(tmp_path, name, task, fuse, save_nii, data_dir, split_dir):
    from efficientq_amd import entrance
    snap = str(tmp_path / name)
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--patch_size", "20,20,18", "--data_dir", data_dir,
            "--split_dir", split_dir, "--test_fp", "--snap_dir", snap]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", fuse]
    if save_nii:
        argv.append("--save_nii")
    entrance.main(argv)
    return snap


@pytest.mark.parametrize("task,fuse", [("lits", None), ("brats", "agg"), ("brats", "con")])
def test_mission_writes_maps_that_reproduce_metrics_csv(tmp_path, task, fuse):
    shape = (20, 24, 18)
    val = ["c1", "c0"]
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy",
                                                train=["c2", "c0"], val=val)
    snap = _run(tmp_path, "with", task, fuse, True, data_dir, split_dir)
    plain = _run(tmp_path, "without", task, fuse, False, data_dir, split_dir)
    for folder in ("fp", "ptq"):
        text = open(os.path.join(snap, folder, "metrics.csv")).read()
        assert text == open(os.path.join(plain, folder, "metrics.csv")).read()
        assert not os.path.exists(os.path.join(plain, folder, "val"))
        rows = {(r["subject"], int(r["class"])): [int(r[k]) for k in ("tp", "fp", "fn", "tn")]
                for r in csv.DictReader(text.splitlines())}
        for sn in val:
            m, hdr = read_nifti(os.path.join(snap, folder, "val", f"{sn}.nii.gz"))
            raw = arrays[sn][1]
            assert m.shape == raw.shape == shape and m.dtype == np.uint16
            assert np.array_equal(hdr["affine"], np.eye(4))
            if task == "lits":
                pred = [m == c for c in range(3)]
                gt = [raw == c for c in range(3)]
            else:
                assert set(np.unique(m)) <= {0, 1, 2, 4}
                pred = [m > 0, (m == 1) | (m == 4), m == 4]
                gt = [raw > 0, (raw == 1) | (raw == 3), raw == 3]
            for c in range(3):
                assert _counts(pred[c], gt[c]) == rows[(sn, c)], (folder, sn, c)
    for i in range(2):
        for tag in ("Qseg", "FPseg"):
            m, _ = read_nifti(os.path.join(snap, f"{tag}{i}.nii.gz"))
            assert m.shape == (16, 16, 16) and m.dtype == np.uint8
            assert int(m.max()) <= 3
            assert not os.path.exists(os.path.join(plain, f"{tag}{i}.nii.gz"))
    assert not os.path.exists(os.path.join(snap, "Qseg2.nii.gz"))
