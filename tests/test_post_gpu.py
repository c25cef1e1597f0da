"""--post end to end on a real MI355X (-m gpu), at the sizes of test_predict_gpu and test_seg_lesions_gpu: the predict
mission's cleaned maps against the numpy restatement applied to the maps the same run writes without --post, and the ptq
mission's metrics_post.csv against tallies recomputed from the maps --save_nii writes.  Integers only: bit for bit."""
import csv
import os

import numpy as np
import pytest
import torch

from efficientq_amd import config as Cf, data as D, entrance, evaluate as E, nifti, predict, synth
from tests import label_clean_ref as R
from tests.test_predict_gpu import _scans
from tests.test_seg_eval_cpu import _args, write_dataset

pytestmark = pytest.mark.gpu
RULES = [((1,), "largest", 0, 0), ((2,), "min", 4, 1)]
POST = ["1:largest", "2:min4>1"]


# ---- predict ------------------------------------------------------------------------------------------------------------
def _checkpoint(root):
    """A seeded random TINY_NET as an FP checkpoint: its maps are speckled enough for both rules to have work."""
    args = Cf.make_args(dict(Cf.TINY_NET, qconv="conv"), 4, 4, merge_type=None)
    QConv, _, kwQ = Cf.get_conv_class(args)
    net = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(net, 0)
    path = os.path.join(root, "state.pkl")
    torch.save({"state_dict": net.state_dict()}, path)
    return args, path


def test_predict_with_post_writes_the_reference_clean_of_the_plain_maps(tmp_path):
    root = str(tmp_path)
    lst = _scans(root, ["b", "a"])
    args, ckpt = _checkpoint(root)
    tables = {}
    for name, post in (("plain", None), ("post", POST)):
        for k, v in dict(src_list=lst, out_dir=os.path.join(root, name), patch_size="32,32,32", prep_mask="nonzero",
                         pretrain=ckpt, post=post).items():
            setattr(args, k, v)
        predict.run(args, window_batch=1)
        with open(os.path.join(root, name, predict.PREDICT_CSV), newline="") as f:
            tables[name] = list(csv.reader(f))
    assert tables["plain"][0] == predict.CSV_HEADER
    assert tables["post"][0] == predict.CSV_HEADER + predict.CSV_POST_COLUMNS
    total = np.zeros(2, dtype=np.int64)
    for r0, r1 in zip(tables["plain"][1:], tables["post"][1:]):
        sn = r1[0]
        before, h0 = nifti.read_nifti(os.path.join(root, "plain", f"{sn}.nii.gz"))
        after, h1 = nifti.read_nifti(os.path.join(root, "post", f"{sn}.nii.gz"))
        want, stats = R.clean(before, RULES, 26)
        assert after.dtype == np.uint8 and after.shape == (40, 44, 36) and np.array_equal(after, want)
        assert np.allclose(h0["affine"], h1["affine"])
        changed = [int(v) for v in r1[-1].split()]
        assert r1[-2] == "1:largest 2:min4>1" and changed == stats[:, 1].tolist()
        # no voxel is relabelled twice (label 1 is cleaned before the second rule adds to it): they are the voxels that differ
        assert sum(changed) == int((before != after).sum())
        k = predict.CSV_HEADER.index("labels")
        assert r0[:k] == r1[:k]
        count = np.bincount(after.ravel())
        assert [int(v) for v in r1[k].split()] == [v for v in range(len(count)) if count[v]]
        assert [int(v) for v in r1[k + 1].split()] == [int(n) for n in count if n]
        total += stats[:, 1]
    assert total.sum() > 0, "the maps gave the rules nothing to do: the test shows nothing"


# ---- the validation -------------------------------------------------------------------------------------------------------
def _ptq(tmp_path, name, task, fuse, data_dir, split_dir, post):
    snap = str(tmp_path / name)
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--patch_size", "20,20,18", "--data_dir", data_dir,
            "--split_dir", split_dir, "--test_fp", "--save_nii", "--snap_dir", snap]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", fuse]
    for rule in post:
        argv += ["--post", rule]
    entrance.main(argv)
    return snap


@pytest.mark.parametrize("task, fuse, post, rules", [
    ("lits", None, POST, RULES),
    ("brats", "agg", ["4:min4>1", "1,2,4:largest"], [((4,), "min", 4, 1), ((1, 2, 4), "largest", 0, 0)]),
])
def test_validation_with_post_scores_the_cleaned_maps_and_leaves_metrics_csv_alone(tmp_path, task, fuse, post, rules):
    shape = (20, 24, 18)
    data_dir, split_dir, _ = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy", train=["c2", "c0"],
                                           val=["c1", "c0"])
    with_post = _ptq(tmp_path, "with", task, fuse, data_dir, split_dir, post)
    plain = _ptq(tmp_path, "without", task, fuse, data_dir, split_dir, [])
    over = dict(merge_type=fuse, patch_size="20,20,18")
    cube = D.get_data_cube(_args(task, data_dir, split_dir, **over))
    truth = {sn: lab[0].numpy().astype(np.uint8) for (_, lab), sn in zip(cube.valloader, cube.val_sn)}
    ncls = 3
    lut = R.class_lut("argmax" if task == "lits" else "brats", ncls)
    head = ["subject", "class", "dsc", "sens", "spec", "acc", "tp", "fp", "fn", "tn", "changed_0", "changed_1"]
    work = 0
    for folder in ("fp", "ptq"):
        same = lambda f: (open(os.path.join(plain, folder, f), "rb").read() ==
                          open(os.path.join(with_post, folder, f), "rb").read())
        assert same("metrics.csv") and not os.path.exists(os.path.join(plain, folder, "metrics_post.csv"))
        for sn in cube.val_sn:          # the --save_nii maps stay the raw decision
            a, b = (nifti.read_nifti(os.path.join(d, folder, "val", f"{sn}.nii.gz"))[0] for d in (plain, with_post))
            assert a.dtype == b.dtype and np.array_equal(a, b)
        with open(os.path.join(with_post, folder, "metrics_post.csv"), newline="") as f:
            table = list(csv.reader(f))
        assert table[0] == head and [(r[0], r[1]) for r in table[1:]] == [(s, str(c)) for s in cube.val_sn
                                                                          for c in range(ncls)]
        for sn in cube.val_sn:
            raw, _ = nifti.read_nifti(os.path.join(with_post, folder, "val", f"{sn}.nii.gz"))
            assert raw.shape == shape and raw.max() <= 4
            want, stats = R.clean(raw.astype(np.uint8), rules, 26)
            counts = R.tallies(want, truth[sn], lut, ncls)
            m = E.metrics_from_counts(torch.from_numpy(counts))
            for c, row in enumerate(r for r in table[1:] if r[0] == sn):
                assert [int(v) for v in row[6:10]] == counts[c].tolist(), (folder, sn, c)
                assert [int(v) for v in row[10:]] == stats[:, 1].tolist()
                assert row[2:6] == ["%.7g" % float(m[k][c]) for k in E.METRICS]
            work += int(stats[:, 1].sum())
    assert work > 0, "the maps gave the rules nothing to do: the test shows nothing"
