"""Validation on labelled volumes on a real MI355X (-m gpu): the window gather / stitch / tally kernels against the
torch path of evaluate.py, validate_seg against the per-window sliding window, and the ptq mission on a tiny
dataset in the reference's layout."""
import csv
import os

import numpy as np
import pytest
import torch

from efficientq_amd import calibrate as K, evaluate as E, synth
from efficientq_amd.hip_ops import from_ndhwc, get_ops
from tests.test_host_cpu import _tiny
from tests.test_seg_eval_cpu import write_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


@pytest.mark.parametrize("C", [4, 3, 1])
def test_gather_equals_image_to_patch3d(ops, C):
    g = torch.Generator().manual_seed(C)
    vol = torch.randn(2, C, 37, 50, 29, generator=g).to(DEV)
    p, o = 16, (4, 6, 2)
    want = E.image_to_patch3d(vol, p, o)
    got = ops.window_gather(vol, p, o)
    assert got.shape == (len(want) * 2, 16, 16, 16, C)
    for w, pt in enumerate(want):
        assert torch.equal(from_ndhwc(got[2 * w:2 * w + 2]), pt), w
    part = ops.window_gather(vol, p, o, first=5, count=7)
    assert torch.equal(part, got[10:24])


@pytest.mark.parametrize("C", [3, 4])
def test_stitch_equals_patch_to_image3d_bitwise(ops, C):
    g = torch.Generator().manual_seed(10 + C)
    N, p, o = 2, 16, (4, 6, 2)
    images = torch.zeros(N, 1, 37, 50, 29, device=DEV)
    nwin = len(E.image_to_patch3d(images, p, o))
    logits = (torch.randn(nwin, N, C, p, p, p, generator=g) * 3).to(DEV)
    logits[0, 0, 0, 0, 0, 0] = -0.0
    want = E.patch_to_image3d(images, list(logits), p, o)
    win = logits.permute(0, 1, 3, 4, 5, 2).reshape(nwin * N, p, p, p, C).contiguous()
    got = ops.window_stitch(win, (N, C, 37, 50, 29), p, o)
    assert torch.equal(got, want)
    # sign of zero included; along h (50, windows of 16, overlap 6: starts 20, 30, 34) voxels 34, 35 have 3 windows
    assert (got.view(torch.int32) == want.view(torch.int32)).all()


def _torch_counts(pred_b, gt_b):
    tp = (pred_b & gt_b).sum()
    fp = (pred_b & ~gt_b).sum()
    fn = (~pred_b & gt_b).sum()
    tn = (~pred_b & ~gt_b).sum()
    return torch.stack([tp, fp, fn, tn])


def _merge_basic(pred, fuse):
    """misc.merge_label_basic."""
    pred = pred.clone()
    if fuse in ("agg", "aggressive"):
        for i in range(len(pred)):
            pred[i] = pred[i:].sum(0) > 0
    elif fuse in ("con", "conservative"):
        for i in range(1, len(pred)):
            pred[i] = pred[i] * pred[i - 1]
    return pred


@pytest.mark.parametrize("shape", [(20, 24, 28), (7, 9, 11)])
def test_tallies_lits_argmax_with_exact_ties(ops, shape):
    g = torch.Generator().manual_seed(3)
    logits = torch.randint(0, 3, (3,) + shape, generator=g).float().to(DEV)   # many exact ties
    label = torch.randint(0, 3, shape, generator=g).to(torch.uint8).to(DEV)
    got = ops.seg_tallies(logits, label, "lits")
    pred = torch.max(logits, 0)[1]
    want = torch.stack([_torch_counts(pred == c, label == c) for c in range(3)])
    assert torch.equal(got, want)


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
def test_tallies_brats_sigmoid_threshold_and_merge(ops, fuse):
    g = torch.Generator().manual_seed(4)
    shape = (3, 18, 20, 22)
    logits = torch.randn(shape, generator=g)
    near = torch.rand(shape, generator=g) < 0.3
    logits[near] = (torch.rand(int(near.sum()), generator=g) * 2 - 1) * 1e-8         # within 1e-8 of 0
    # every float from 2^12 ulps below to 2^12 ulps above the framework's threshold
    t = ops.sigmoid_threshold()
    tb = int(torch.tensor([-t]).view(torch.int32))
    sweep = -torch.arange(tb - 4096, tb + 4096, dtype=torch.int32).view(torch.float32)
    flat = logits.view(-1)
    flat[:sweep.numel()] = sweep
    logits = logits.to(DEV)
    label = (torch.rand(shape, generator=g) < 0.4).to(torch.uint8).to(DEV)
    got = ops.seg_tallies(logits, label, "brats", fuse)
    pred = _merge_basic((torch.sigmoid(logits) >= 0.5).int(), fuse).bool()
    want = torch.stack([_torch_counts(pred[c], label[c].bool()) for c in range(3)])
    assert torch.equal(got, want)
    assert t < 0 and (torch.sigmoid(torch.tensor([t], device=DEV)) >= 0.5).item()
    print(f"fp32 sigmoid(x) >= 0.5 on the device from x = {t!r}")


def _loader(vols, labels):
    return list(zip([v[None] for v in vols], [l[None] for l in labels]))


def test_validate_seg_matches_the_per_window_loop(gold):
    """g6d-style width 32,64,32 LiTS net, calibrated: batched windows + HIP stitch + tallies against
    sliding_window_forward + torch counts.  A batch of windows may round a logit differently from one window alone;
    only voxels whose decision margin (top-1 minus top-2 logit) is below 1e-5 may then be counted differently."""
    g = gold("g6d_wide_lits_L4.npz")
    args, model, _ = _tiny("lits", width="32,64,32")
    synth.randomise_network(model, int(g["net_seed"]))
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_name(model)
    gen = torch.Generator().manual_seed(5)
    K.calibrate_model(model, torch.randn(2, 1, 16, 16, 16, generator=gen).to(DEV), "lits", args.init_stride)
    K.set_quantized(model)
    shape = (30, 36, 28)
    vols = [torch.randn(1, *shape, generator=gen) for _ in range(2)]
    labels = [torch.randint(0, 3, shape, generator=gen) for _ in range(2)]
    p, o = (16, 16, 16), (4, 6, 2)
    for wb in (3, None):
        res = E.validate_seg(model, _loader(vols, labels), "lits", p, o, window_batch=wb, names=["a", "b"])
        assert [r["name"] for r in res] == ["a", "b"]
        for r, v, lab in zip(res, vols, labels):
            out = E.sliding_window_forward(model, v[None].to(DEV), p, o)[-1][0]
            pred = torch.max(out, 0)[1]
            lab_d = lab.to(DEV)
            want = torch.stack([_torch_counts(pred == c, lab_d == c) for c in range(3)]).cpu()
            top2 = torch.topk(out, 2, dim=0).values
            low = int(((top2[0] - top2[1]) < 1e-5).sum())
            diff = int((r["counts"] - want).abs().sum())
            print(f"window_batch={wb}: {low} voxels with a margin below 1e-5, counts differ by {diff}")
            assert diff <= 2 * low
            if diff == 0:
                m = E.metrics_from_counts(want)
                for k in E.METRICS:
                    assert torch.equal(r[k], m[k])
            # torch's own metrics on the masks
            for c in range(3):
                assert float(r["dsc"][c]) == pytest.approx(float(E.dice(pred == c, lab_d == c)), abs=2 * low / lab.numel() + 1e-6)


@pytest.mark.parametrize("task", ["lits", "brats"])
def test_ptq_mission_on_labelled_volumes_writes_metrics(tmp_path, task):
    from efficientq_amd import entrance
    data_dir, split_dir, _ = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], (20, 24, 18), "npy",
                                           train=["c2", "c0"], val=["c1", "c0"])
    snap = str(tmp_path / "snap")
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--patch_size", "20,20,18", "--data_dir", data_dir,
            "--split_dir", split_dir, "--test_fp", "--snap_dir", snap]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", "agg"]
    entrance.main(argv)
    for folder in ("fp", "ptq"):
        rows = list(csv.DictReader(open(os.path.join(snap, folder, "metrics.csv"))))
        assert [(r["subject"], r["class"]) for r in rows] == [(s, str(c)) for s in ("c0", "c1") for c in range(3)]
        for r in rows:
            n = sum(int(r[k]) for k in ("tp", "fp", "fn", "tn"))
            assert n == 20 * 24 * 18
            assert 0.0 <= float(r["dsc"]) <= 1.0 and float(r["acc"]) == pytest.approx(
                (int(r["tp"]) + int(r["tn"])) / n, rel=1e-6)
    for f in ("layer_loss.txt", "state_in_int8.pkl"):
        assert os.path.exists(os.path.join(snap, f))
