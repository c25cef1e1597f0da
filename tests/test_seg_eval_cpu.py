"""Labelled-volume validation, host side (no GPU): the data layout reader (efficientq_amd/data.py), the metric
formulas and the CSV writer of evaluate.py, and the C-ABI rows of the three validation kernels."""
import argparse
import csv
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, calibrate as K, config as Cf, data as D, evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_dataset(root, task, subjects, shape, access_type="npy", seed=0, train=None, val=None):
    """A tiny dataset in the reference's layout; returns (data_dir, split_dir, {subject: (image, label)})."""
    rng = np.random.default_rng(seed)
    data_dir, split_dir = os.path.join(root, "data"), os.path.join(root, "split")
    mods = D.MODALITIES[task]
    nlab = 4 if task == "brats" else 3
    arrays = {}
    for sn in subjects:
        img = rng.standard_normal((len(mods),) + tuple(shape)).astype(np.float32)
        lab = rng.integers(0, nlab, size=shape).astype(np.uint8)
        arrays[sn] = (img, lab)
        for m, a in list(zip(mods, img)) + [("seg", lab)]:
            os.makedirs(os.path.join(data_dir, m), exist_ok=True)
            if access_type == "npy":
                np.save(os.path.join(data_dir, m, f"{sn}.npy"), a)
            else:
                np.savez(os.path.join(data_dir, m, f"{sn}.npz"), a)
    os.makedirs(os.path.join(split_dir, "round1"), exist_ok=True)
    for name, lst in (("train", train if train is not None else subjects), ("val", val if val is not None else subjects)):
        with open(os.path.join(split_dir, "round1", f"{name}.txt"), "w") as f:
            f.write("\n".join(lst) + "\n")
    return data_dir, split_dir, arrays


def _args(task, data_dir, split_dir, **over):
    net = Cf.TINY_NET if task == "lits" else dict(Cf.TINY_NET, task="brats", nMod=4, nClass=4, multi_label="brats")
    a = Cf.make_args(net, 4, 4, data_dir=data_dir, split_dir=split_dir, access_type="npy", merge_type=None,
                     patch_size=None)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("access_type", ["npy", "npz"])
def test_lits_cube_reads_the_layout_in_sorted_subject_order(tmp_path, access_type):
    subjects = ["case_c", "case_a", "case_b"]
    data_dir, split_dir, arr = write_dataset(str(tmp_path), "lits", subjects, (6, 5, 4), access_type,
                                             val=["case_b", "", "case_a"])
    cube = D.get_data_cube(_args("lits", data_dir, split_dir, access_type=access_type))
    assert cube.train_sn == ["case_a", "case_b", "case_c"] and cube.val_sn == ["case_a", "case_b"]
    assert cube.patch_size == (128, 128, 64) and cube.overlap == 16
    cube.trainseqloader.dataset.use_fix_transform()
    got = list(cube.trainseqloader)
    assert len(got) == 3
    for (img, lab), sn in zip(got, cube.train_sn):
        assert img.dtype == torch.float32 and img.shape == (1, 1, 6, 5, 4)
        assert lab.dtype == torch.int64 and lab.shape == (1, 6, 5, 4)
        assert torch.equal(img[0], torch.from_numpy(arr[sn][0]))
        assert torch.equal(lab[0], torch.from_numpy(arr[sn][1]).long())
    assert [sn for sn in cube.val_sn] == ["case_a", "case_b"] and len(list(cube.valloader)) == 2


def test_brats_cube_splits_the_label_into_nested_channels(tmp_path):
    data_dir, split_dir, arr = write_dataset(str(tmp_path), "brats", ["s1", "s0"], (3, 4, 5), "npz")
    cube = D.get_data_cube(_args("brats", data_dir, split_dir, access_type="npz", patch_size="16,8,8"))
    assert cube.patch_size == (16, 8, 8)
    img, lab = next(iter(cube.valloader))
    raw = torch.from_numpy(arr["s0"][1]).long()
    assert img.shape == (1, 4, 3, 4, 5) and torch.equal(img[0], torch.from_numpy(arr["s0"][0]))
    assert lab.shape == (1, 3, 3, 4, 5) and lab.dtype == torch.float32
    assert torch.equal(lab[0, 0], (raw > 0).float())
    assert torch.equal(lab[0, 1], ((raw == 1) | (raw == 3)).float())
    assert torch.equal(lab[0, 2], (raw == 3).float())
    # lits split and the binary label
    lits = D.label_transform(None, "lits")(raw)
    assert torch.equal(lits, torch.stack([raw > 0, raw == 2]).float())
    assert torch.equal(D.label_transform("1", None)(raw), (raw > 0).long())
    assert D.label_transform("1", "brats") is D.label_split_brats


def test_calibration_takes_the_train_split_in_order_with_dataid_and_batchsz(tmp_path):
    subjects = ["b", "d", "a", "c"]
    data_dir, split_dir, arr = write_dataset(str(tmp_path), "lits", subjects, (8, 8, 8))
    cube = D.get_data_cube(_args("lits", data_dir, split_dir))
    args = _args("lits", data_dir, split_dir, lwq_dataid=1, lwq_batchsz=2, lwq_patchsz="4,4,4")
    data, label = K.get_calibration_data(args, cube)
    want = [K.center_crop(torch.from_numpy(arr[sn][0])[None], [4, 4, 4]) for sn in ("b", "c")]
    assert torch.equal(data, torch.cat(want, 0))
    assert label.shape == (2, 4, 4, 4)
    args = _args("lits", data_dir, split_dir, lwq_dataid=3, lwq_batchsz=1, lwq_patchsz="8,8,8")
    data, _ = K.get_calibration_data(args, cube)
    assert torch.equal(data[0], torch.from_numpy(arr["d"][0]))


def test_missing_files_and_unknown_access_type_raise(tmp_path):
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "lits", ["a"], (2, 2, 2))
    with pytest.raises(RuntimeError):
        D.SegVolumes(data_dir, ["a"], ("ct",), "memmap")
    ds = D.SegVolumes(data_dir, ["zz"], ("ct",), "npy")
    with pytest.raises(FileNotFoundError):
        ds[0]


def test_parser_has_access_type_and_merge_type():
    a = Cf.build_parser().parse_args(["ptq"])
    assert a.access_type == "npy" and a.merge_type is None
    a = Cf.build_parser().parse_args(["ptq", "--access_type", "npz", "--merge_type", "agg"])
    assert a.access_type == "npz" and a.merge_type == "agg"


def test_metric_formulas_against_hand_counts():
    # class 0: TP 3, FP 1, FN 2, TN 4 ; class 1: nothing predicted, nothing labelled
    counts = torch.tensor([[3, 1, 2, 4], [0, 0, 0, 10]])
    m = E.metrics_from_counts(counts)
    eps = 1e-6
    assert float(m["dsc"][0]) == pytest.approx((6 + eps) / (4 + 5 + eps), rel=1e-6)
    assert float(m["sens"][0]) == pytest.approx((3 + eps) / (5 + eps), rel=1e-6)
    assert float(m["spec"][0]) == pytest.approx((4 + eps) / (5 + eps), rel=1e-6)
    assert float(m["acc"][0]) == pytest.approx(7 / 10, rel=1e-6)
    assert [float(m[k][1]) for k in E.METRICS] == [1.0, 1.0, 1.0, 1.0]
    # the same fp32 numbers metrics.py computes on the binary masks
    pred = torch.tensor([1, 1, 1, 1, 0, 0, 0, 0, 0, 0])
    gt = torch.tensor([1, 1, 1, 0, 1, 1, 0, 0, 0, 0])
    assert torch.equal(m["dsc"][0], E.dice(pred, gt))
    sens = ((pred * gt).sum().float() + eps) / (gt.sum().float() + eps)
    spec = (((1 - pred) * (1 - gt)).sum().float() + eps) / ((1 - gt).sum().float() + eps)
    acc = (pred == gt).sum().float() / torch.tensor(gt.numel(), dtype=torch.float)
    assert torch.equal(m["sens"][0], sens) and torch.equal(m["spec"][0], spec) and torch.equal(m["acc"][0], acc)


def test_metrics_csv_has_one_row_per_subject_and_class(tmp_path):
    res = []
    for name, counts in (("s1", torch.tensor([[3, 1, 2, 4], [1, 0, 0, 9]])), ("s2", torch.tensor([[0, 2, 0, 8], [5, 0, 5, 0]]))):
        r = {"name": name, "counts": counts}
        r.update(E.metrics_from_counts(counts))
        res.append(r)
    path = str(tmp_path / "metrics.csv")
    E.write_metrics_csv(path, res)
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["subject", "class", "dsc", "sens", "spec", "acc", "tp", "fp", "fn", "tn"]
    assert [r[:2] for r in rows[1:]] == [["s1", "0"], ["s1", "1"], ["s2", "0"], ["s2", "1"]]
    assert rows[4][6:] == ["5", "0", "5", "0"] and float(rows[4][3]) == pytest.approx(0.5, rel=1e-6)
    means = E.metric_means(res)
    assert float(means["acc"][0]) == pytest.approx((0.7 + 0.8) / 2, rel=1e-6)


def test_validation_symbols_in_header_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("effq_window_gather", "effq_window_stitch", "effq_seg_tallies"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    ws = re.search(r"#define EFFQ_SEG_TALLIES_WS_BYTES \((\d+) \* 3 \* EFFQ_SEG_TALLIES_MAX_CLASSES \* 4\)", hdr)
    mc = re.search(r"#define EFFQ_SEG_TALLIES_MAX_CLASSES (\d+)", hdr)
    assert int(mc.group(1)) == _lib.SEG_TALLIES_MAX_CLASSES
    assert int(ws.group(1)) * 3 * _lib.SEG_TALLIES_MAX_CLASSES * 4 == _lib.SEG_TALLIES_WS_BYTES


def test_window_grid_matches_window_starts():
    from efficientq_amd.hip_ops import HipOps
    for size, p, o in ((37, 16, 4), (50, 16, 6), (29, 16, 2), (16, 16, 0), (155, 128, 16), (240, 128, 16)):
        assert HipOps.window_grid((size,) * 3, p, o) == (len(E.window_starts(size, p, o)),) * 3
    with pytest.raises(_lib.EffqError):
        HipOps.window_grid((8, 8, 8), 16, 4)
    with pytest.raises(_lib.EffqError):
        HipOps.window_grid((32, 32, 32), 16, 16)
