"""Validation against the FP network on a real MI355X (-m gpu): effq_seg_agreement against a torch reference (the
decisions as test_seg_eval_gpu takes them, the sums, the sigmoid and the softmax in fp64 on the CPU) and against the
existing kernels, validate_seg(fp_model=...) on the tiny network, and the ptq mission with --vs_fp / --unlabelled.

The bars.  counts, flips, the map and max |q - f| are exact: integers, and the rounded fp64 difference of two floats,
whose maximum does not depend on any order.  The two sums of squares lie within a relative n 2^-52 of the reference, n
the number of terms: any order of summing n non-negative terms is within (n - 1) 2^-53 relative of the exact sum, once
more for the rounding of the terms.  prob_mae lies within an absolute 1e-12: each fp64 probability is within a few
2^-53 of the host's, the bar is three orders above that and far below any value of interest."""
import copy
import csv
import os
import shutil

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, calibrate as K, evaluate as E, synth
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.nifti import read_nifti
from tests.test_host_cpu import _tiny
from tests.test_seg_eval_cpu import write_dataset
from tests.test_seg_eval_gpu import _merge_basic, _torch_counts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _decisions(x, mode, fuse):
    """C x spatial bool, on the device: torch.max for argmax, the framework's fp32 sigmoid >= 0.5 merged by `fuse`."""
    if mode == "argmax":
        best = torch.max(x, 0)[1]
        return torch.stack([best == c for c in range(x.shape[0])])
    return _merge_basic((torch.sigmoid(x) >= 0.5).int(), fuse).bool()


def _reference(q, f, mode, fuse):
    C = q.shape[0]
    dq, df = _decisions(q, mode, fuse), _decisions(f, mode, fuse)
    counts = torch.stack([_torch_counts(dq[c], df[c]) for c in range(C)]).cpu()
    diff = (dq ^ df).cpu()
    vmap = torch.zeros(diff.shape[1:], dtype=torch.int64)
    for c in range(C):
        vmap |= diff[c].long() << c
    q64, f64 = q.cpu().double().reshape(C, -1), f.cpu().double().reshape(C, -1)
    d = q64 - f64
    if mode == "argmax":
        dp = torch.softmax(q64, 0) - torch.softmax(f64, 0)
    else:
        dp = torch.sigmoid(q64) - torch.sigmoid(f64)
    return dict(counts=counts, flips=int((vmap != 0).sum()), map=vmap.to(torch.uint8), ssd=(d * d).sum(1),
                sff=(f64 * f64).sum(1), max=d.abs().max(1).values, mae=dp.abs().sum(1) / d.shape[1])


def _check(ops, q, f, mode, fuse=None):
    """One call against the reference, at the bars of the module docstring; returns what the kernel gave."""
    want = _reference(q, f, mode, fuse)
    counts, flips, stats, vmap = ops.seg_agreement(q, f, mode, fuse, want_map=True)
    nomap = ops.seg_agreement(q, f, mode, fuse)
    assert nomap[3] is None and torch.equal(nomap[0], counts) and torch.equal(nomap[1], flips)
    assert torch.equal(nomap[2].view(torch.int64), stats.view(torch.int64))
    S = q[0].numel()
    stats = stats.cpu()
    print(f"{mode} fuse={fuse} C={q.shape[0]} S={S}: flips {int(flips)} / {want['flips']}, sum (q-f)^2 rel err "
          f"{((stats[:, 0] - want['ssd']).abs() / want['ssd'].clamp_min(1e-300)).max():.3g}, sum f^2 rel err "
          f"{((stats[:, 1] - want['sff']).abs() / want['sff'].clamp_min(1e-300)).max():.3g}, prob_mae abs err "
          f"{(stats[:, 3] / S - want['mae']).abs().max():.3g} (bars {S * 2.0 ** -52:.3g}, 1e-12)")
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), want["counts"])
    assert (counts.sum(1) == S).all()
    assert flips.shape == (1,) and int(flips) == want["flips"]
    assert vmap.dtype == torch.uint8 and vmap.shape == q.shape[1:] and torch.equal(vmap.cpu(), want["map"])
    assert torch.equal(stats[:, 2], want["max"])
    bar = S * 2.0 ** -52
    assert ((stats[:, 0] - want["ssd"]).abs() <= bar * want["ssd"]).all()
    assert ((stats[:, 1] - want["sff"]).abs() <= bar * want["sff"]).all()
    assert ((stats[:, 3] / S - want["mae"]).abs() <= 1e-12).all()
    return counts, flips, stats, vmap


def _extreme(q, f, c=0):
    """One pair far from all others, for the maximum: 1.5e3 against -2.5e3 at the last voxel of class c."""
    q.view(q.shape[0], -1)[c, -1] = 1.5e3
    f.view(f.shape[0], -1)[c, -1] = -2.5e3


@pytest.mark.parametrize("shape", [(7, 9, 11), (20, 24, 28)])
def test_agreement_argmax_with_exact_ties(ops, shape):
    g = torch.Generator().manual_seed(3)
    q = torch.randint(0, 3, (3,) + shape, generator=g).float()      # many exact ties
    f = torch.randint(0, 3, (3,) + shape, generator=g).float()
    _extreme(q, f, 1)
    _, flips, stats, _ = _check(ops, q.to(DEV), f.to(DEV), "argmax")
    assert int(flips) > 0 and float(stats[1, 2]) == 4000.0


def test_agreement_argmax_one_class(ops):
    g = torch.Generator().manual_seed(5)
    q, f = torch.randn(1, 7, 9, 11, generator=g), torch.randn(1, 7, 9, 11, generator=g)
    _extreme(q, f)
    counts, flips, stats, vmap = _check(ops, q.to(DEV), f.to(DEV), "argmax")
    assert counts.tolist() == [[693, 0, 0, 0]] and int(flips) == 0 and float(stats[0, 3]) == 0.0 and not vmap.any()


def _sigmoid_case(ops, shape, seed):
    """Logits around 0 with, in both networks at different voxels, the threshold itself and the float just below it."""
    g = torch.Generator().manual_seed(seed)
    q, f = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    t = torch.tensor(ops.sigmoid_threshold(), dtype=torch.float32)
    below = torch.nextafter(t, torch.tensor(-1.0))
    assert float(below) < float(t) < 0
    for x, off in ((q, 0), (f, 1)):
        flat = x.view(-1)
        flat[off::7] = t
        flat[off + 2::7] = below
    near = torch.rand(shape, generator=g) < 0.2
    f[near] = q[near] + 1e-3 * torch.randn(int(near.sum()), generator=g)      # voxels where the networks nearly agree
    _extreme(q, f, shape[0] - 1)
    return q.to(DEV), f.to(DEV)


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
def test_agreement_sigmoid_threshold_and_merge(ops, fuse):
    q, f = _sigmoid_case(ops, (3, 18, 20, 22), 4)
    counts, flips, _, _ = _check(ops, q, f, "sigmoid", fuse)
    assert int(flips) > 0 and (counts[:, 1] > 0).all() and (counts[:, 2] > 0).all()


@pytest.mark.parametrize("fuse", [None, "con"])
def test_agreement_sigmoid_eight_classes(ops, fuse):
    q, f = _sigmoid_case(ops, (8, 7, 9, 11), 6)
    _, _, _, vmap = _check(ops, q, f, "sigmoid", fuse)
    assert int(vmap.max()) >= 128                                   # the bit of class 7 is used


def test_agreement_over_more_than_one_grid_sweep_with_a_tail(ops):
    """S = 2^20 + 3: the workgroups walk their grid-stride loop more than once, three voxels are left to the scalar tail
    and the channel planes do not start on 16 B.  The extreme pair is 3e38 against -3e38: |q - f| = 6e38 exists in fp64
    only."""
    S = 2 ** 20 + 3
    g = torch.Generator().manual_seed(7)
    q = torch.randn(3, S, generator=g)
    f = q + 0.3 * torch.randn(3, S, generator=g)
    q[0, S - 2], f[0, S - 2] = 3e38, -3e38
    counts, flips, stats, vmap = _check(ops, q.to(DEV), f.to(DEV), "argmax")
    big = float(np.float32(3e38))
    assert float(stats[0, 2]) == 2 * big and 2 * big > float(np.finfo(np.float32).max)
    assert 0 < int(flips) < S and vmap.shape == (S,)
    # the same case in sigmoid mode (the fp64 exponentials of every voxel), without the pair that swamps class 0
    q[0, S - 2], f[0, S - 2] = 1.0, -1.0
    _check(ops, q.to(DEV), f.to(DEV), "sigmoid", "agg")


@pytest.mark.parametrize("mode,fuse", [("argmax", None), ("sigmoid", None), ("sigmoid", "agg")])
def test_agreement_of_identical_inputs_is_total(ops, mode, fuse):
    q = torch.randn(3, 9, 10, 13, generator=torch.Generator().manual_seed(8)).to(DEV)
    counts, flips, stats, vmap = ops.seg_agreement(q, q.clone(), mode, fuse, want_map=True)
    assert int(flips) == 0 and not vmap.any()
    assert (counts[:, 1] == 0).all() and (counts[:, 2] == 0).all() and (counts.sum(1) == 9 * 10 * 13).all()
    stats = stats.cpu()
    assert (stats[:, 0] == 0).all() and (stats[:, 2] == 0).all() and (stats[:, 3] == 0).all()
    assert (stats[:, 1] > 0).all()


def test_agreement_is_deterministic(ops):
    g = torch.Generator().manual_seed(9)
    q = torch.randn(3, 2 ** 18 + 1, generator=g).to(DEV)
    f = (q + 0.5 * torch.randn(3, 2 ** 18 + 1, generator=g).to(DEV)).contiguous()
    for mode in ("argmax", "sigmoid"):
        a = ops.seg_agreement(q, f, mode)
        b = ops.seg_agreement(q, f, mode)
        assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode,fuse", [("argmax", None), ("sigmoid", None), ("sigmoid", "agg"), ("sigmoid", "con")])
def test_agreement_counts_equal_the_tallies_against_the_fp_label_map(ops, mode, fuse):
    q, f = _sigmoid_case(ops, (3, 18, 20, 22), 10)
    if mode == "argmax":
        q, f = torch.round(q * 2), torch.round(f * 2)             # ties
        label = ops.seg_labels(f[None], "argmax")[0]
        want = ops.seg_tallies(q, label, "lits")
    else:
        label = ops.seg_labels(f[None], "planes", fuse)[0]
        want = ops.seg_tallies(q, label, "brats", fuse)
    assert torch.equal(ops.seg_agreement(q, f, mode, fuse)[0], want)


def test_agreement_refuses_bad_arguments_before_any_launch(ops):
    q = torch.randn(3, 4, 5, 6, device=DEV)
    with pytest.raises(_lib.EffqError):
        ops.seg_agreement(q, q[:, :3], "argmax")                      # shapes
    with pytest.raises(_lib.EffqError):
        ops.seg_agreement(q, q.double(), "argmax")                    # fp32
    with pytest.raises(_lib.EffqError):
        ops.seg_agreement(q, q.transpose(1, 2).contiguous().transpose(1, 2), "argmax")    # contiguous
    with pytest.raises(_lib.EffqError):
        ops.seg_agreement(q, q.cpu(), "argmax")                       # same device
    with pytest.raises(_lib.EffqError):
        ops.seg_agreement(torch.randn(9, 8, device=DEV), torch.randn(9, 8, device=DEV), "sigmoid")   # class limit
    with pytest.raises(_lib.EffqError):
        ops.seg_agreement(q, q, "argmax", "agg")                      # a merge needs the sigmoid mode
    with pytest.raises(_lib.EffqError):
        ops.seg_agreement(q, q, "softmax")


# ---- validate_seg -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pair():
    """The tiny LiTS network calibrated at 4 / 4 levels, and the copy of it taken before the calibration."""
    args, model, _ = _tiny("lits")
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_name(model)
    fp = copy.deepcopy(model)
    K.set_fp(fp)
    gen = torch.Generator().manual_seed(5)
    K.calibrate_model(model, torch.randn(2, 1, 16, 16, 16, generator=gen).to(DEV), "lits", args.init_stride)
    K.set_quantized(model)
    vol = torch.randn(1, 40, 48, 36, generator=gen)
    label = torch.randint(0, 3, (40, 48, 36), generator=gen)
    return model, fp, vol, label


def _stitched(ops, net, vol, p, o, wb):
    """The stitched last-head logits of one network on its own, in validate_seg's batches of `wb` windows."""
    from efficientq_amd.hip_ops import from_ndhwc
    v = vol[None].to(DEV)
    nwin = int(np.prod(ops.window_grid(v.shape[-3:], (p,) * 3, (o,) * 3)))
    outs = []
    with torch.no_grad():
        for first in range(0, nwin, wb):
            x = from_ndhwc(ops.window_gather(v, p, o, first, min(wb, nwin - first)))
            outs.append(E._last_head(net(x)).permute(0, 2, 3, 4, 1))
    win = torch.cat(outs).contiguous()
    return ops.window_stitch(win, (1, int(win.shape[-1])) + tuple(v.shape[-3:]), p, o)[0]


def test_validate_seg_vs_fp_equals_the_kernel_on_separately_stitched_logits(ops, tiny_pair):
    """40 x 48 x 36 in windows of 32 with overlap 8: eight windows in batches of three.  As test_seg_eval_gpu holds
    validate_seg to the per-window path: a forward of its own may round a logit differently, and only voxels whose
    decision margin (top-1 minus top-2 logit, in either network) is below 1e-5 may then be counted differently; where no
    count differs the metrics are the same bits.  The drift sums are smooth in the logits: a logit that moves by a few
    fp32 ulps (2^-24 relative) moves them by parts in 1e6, so 1e-4 relative holds them."""
    model, fp, vol, label = tiny_pair
    p, o, wb = 32, 8, 3
    loader = [(vol[None], label[None])]
    res = E.validate_seg(model, loader, "lits", p, o, window_batch=wb, names=["a"], fp_model=fp, lesions=True,
                         surface=True)
    plain = E.validate_seg(model, loader, "lits", p, o, window_batch=wb, names=["a"], lesions=True, surface=True)
    # every other entry is what it is without fp_model
    assert set(res[0]) == set(plain[0]) | {"vs_fp"}
    for k, v in plain[0].items():
        assert torch.equal(res[0][k], v) if torch.is_tensor(v) else res[0][k] == v, k
    q, f = _stitched(ops, model, vol, p, o, wb), _stitched(ops, fp, vol, p, o, wb)
    counts, flips, stats, _ = ops.seg_agreement(q, f, "argmax")
    counts, stats, S = counts.cpu(), stats.cpu(), q[0].numel()
    vs = res[0]["vs_fp"]
    low = 0
    for x in (q, f):
        top2 = torch.topk(x, 2, dim=0).values
        low += int(((top2[0] - top2[1]) < 1e-5).sum())
    diff = int((vs["counts"] - counts).abs().sum())
    print(f"{low} voxels with a margin below 1e-5, counts differ by {diff}, flips {vs['flips']} of {S}, "
          f"dsc {vs['dsc'].tolist()}, logit_rel_mse {vs['logit_rel_mse'].tolist()}, prob_mae {vs['prob_mae'].tolist()}")
    assert diff <= 2 * low and abs(vs["flips"] - int(flips)) <= low
    assert vs["flip_frac"] == vs["flips"] / S and 0 < vs["flips"] < S
    if diff == 0:
        assert vs["flips"] == int(flips)
        m = E.metrics_from_counts(counts)
        for k in E.METRICS:
            assert torch.equal(vs[k], m[k])
    assert torch.allclose(vs["logit_rel_mse"], stats[:, 0] / stats[:, 1], rtol=1e-4, atol=0)
    assert torch.allclose(vs["logit_max"], stats[:, 2], rtol=1e-4, atol=0)
    assert torch.allclose(vs["prob_mae"], stats[:, 3] / S, rtol=1e-4, atol=0)
    # the lesion and surface entries are the existing ops against the FP decisions
    lab = ops.seg_labels(f[None], "argmax")[0]
    if diff == 0:
        assert torch.equal(vs["lesions"], ops.seg_lesions(q, lab, "lits").cpu())
        sc, ss = ops.seg_surface(q, lab, "lits")
        assert torch.equal(vs["surface_counts"], sc.cpu())
        assert torch.equal(vs["surface"], E.surface_metrics(sc, ss, (40, 48, 36)))
    assert vs["lesions"].shape == (3, 4) and vs["surface"].shape == (3, 3) and "surface_unit" not in vs


def test_validate_seg_against_itself_agrees_totally_and_unlabelled_cases(tiny_pair):
    model, fp, vol, label = tiny_pair
    res = E.validate_seg(model, [(vol[None], label[None])], "lits", 32, 8, window_batch=3, fp_model=model)
    vs = res[0]["vs_fp"]
    assert vs["flips"] == 0 and vs["flip_frac"] == 0.0
    assert (vs["counts"][:, 1:3] == 0).all() and (vs["counts"].sum(1) == vol.numel()).all()
    assert (vs["logit_rel_mse"] == 0).all() and (vs["logit_max"] == 0).all() and (vs["prob_mae"] == 0).all()
    # an empty label: name and vs_fp only, the same vs_fp as with the label; without fp_model a RuntimeError naming it
    empty = torch.empty(1, 0, dtype=torch.uint8)
    un = E.validate_seg(model, [(vol[None], empty)], "lits", 32, 8, window_batch=3, names=["nolab"], fp_model=fp)
    lab = E.validate_seg(model, [(vol[None], label[None])], "lits", 32, 8, window_batch=3, names=["lab"], fp_model=fp)
    assert set(un[0]) == {"name", "vs_fp"} and un[0]["name"] == "nolab"
    assert torch.equal(un[0]["vs_fp"]["counts"], lab[0]["vs_fp"]["counts"])
    assert torch.equal(un[0]["vs_fp"]["prob_mae"], lab[0]["vs_fp"]["prob_mae"])
    with pytest.raises(RuntimeError, match="nolab"):
        E.validate_seg(model, [(vol[None], empty)], "lits", 32, 8, window_batch=3, names=["nolab"])


# ---- the mission --------------------------------------------------------------------------------------------------
def _argv(task, data_dir, split_dir, snap):
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--snap_dir", snap]
    if data_dir is not None:
        argv += ["--patch_size", "20,20,18", "--data_dir", data_dir, "--split_dir", split_dir]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", "agg"]
    return argv


def _agreement_rows(snap, subjects, ncls, voxels):
    rows = list(csv.DictReader(open(os.path.join(snap, "ptq", "agreement.csv"))))
    assert [(r["subject"], r["class"]) for r in rows] == [(s, str(c)) for s in subjects for c in range(ncls)]
    for r in rows:
        n = [int(r[k]) for k in E.AGREEMENT_COUNTS]
        assert sum(n) == voxels and 0.0 <= float(r["dsc"]) <= 1.0
        assert float(r["flip_frac_class"]) == pytest.approx((n[1] + n[2]) / voxels, rel=1e-6)
        assert float(r["logit_rel_mse"]) > 0 and float(r["logit_max"]) > 0 and 0 < float(r["prob_mae"]) < 1
    return rows


def test_ptq_mission_with_vs_fp_writes_the_agreement_and_the_maps(tmp_path, capsys):
    from efficientq_amd import entrance
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "lits", ["c2", "c0", "c1"], (20, 24, 18), "npy",
                                           train=["c2", "c0"], val=["c1", "c0"])
    snap = str(tmp_path / "snap")
    entrance.main(_argv("lits", data_dir, split_dir, snap) + ["--vs_fp", "--save_nii", "--is_cc", "--test_fp"])
    rows = _agreement_rows(snap, ("c0", "c1"), 3, 20 * 24 * 18)
    assert list(rows[0])[-4:] == list(E.LESION_COLUMNS)
    for sn in ("c0", "c1"):
        a, _ = read_nifti(os.path.join(snap, "ptq", "val_vs_fp", f"{sn}.nii.gz"))
        assert a.dtype == np.uint8 and a.shape == (20, 24, 18) and a.max() < 8
        flipped = int((a != 0).sum())
        per_class = [int(r["q_only"]) + int(r["fp_only"]) for r in rows if r["subject"] == sn]
        assert [int(((a >> c) & 1).sum()) for c in range(3)] == per_class and flipped <= sum(per_class)
        assert os.path.exists(os.path.join(snap, "ptq", "val", f"{sn}.nii.gz"))
    # the label-side outputs are there as before, and the fp folder knows nothing of the switch
    assert os.path.exists(os.path.join(snap, "ptq", "metrics.csv"))
    assert sorted(os.listdir(os.path.join(snap, "fp"))) == ["metrics.csv", "val"]
    out = capsys.readouterr().out
    assert "against the FP network" in out and "prob_mae" in out


def test_ptq_mission_on_unlabelled_volumes(tmp_path):
    from efficientq_amd import entrance
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "brats", ["c2", "c0", "c1"], (20, 24, 18), "npy",
                                           train=["c2", "c0"], val=["c1", "c0"])
    shutil.rmtree(os.path.join(data_dir, "seg"))
    snap = str(tmp_path / "snap")
    entrance.main(_argv("brats", data_dir, split_dir, snap) + ["--vs_fp", "--unlabelled", "--surf_dist"])
    rows = _agreement_rows(snap, ("c0", "c1"), 3, 20 * 24 * 18)
    assert list(rows[0])[-3:] == list(E.SURFACE_COLUMNS)
    assert not os.path.exists(os.path.join(snap, "ptq", "metrics.csv"))
    assert os.path.exists(os.path.join(snap, "state_in_int8.pkl"))


def test_synthetic_mission_with_vs_fp_ends_with_a_number(tmp_path, capsys):
    from efficientq_amd import entrance
    snap = str(tmp_path / "snap")
    entrance.main(_argv("lits", None, None, snap) + ["--synthetic", "--vs_fp"])
    _agreement_rows(snap, ("synth2", "synth3"), 3, 16 ** 3)
    assert not os.path.exists(os.path.join(snap, "ptq", "metrics.csv"))
    assert "against the FP network" in capsys.readouterr().out
