"""Validation against the FP network (--vs_fp, --unlabelled), host side (no GPU): the switches and their YAML keys, the
combinations entrance.check_switches refuses, the C-ABI row of effq_seg_agreement, the dataset without seg/ and
agreement.csv."""
import csv
import os
import re
import shutil

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, data as D, entrance, evaluate as E
from tests.test_seg_eval_cpu import write_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the switches -------------------------------------------------------------------------------------------------
def test_parser_knows_both_switches_and_yaml_keys_set_them(tmp_path):
    a = Cf.build_parser().parse_args(["ptq"])
    assert a.vs_fp is False and a.unlabelled is False
    a = Cf.build_parser().parse_args(["ptq", "--vs_fp", "--unlabelled"])
    assert a.vs_fp is True and a.unlabelled is True
    m = Cf.make_args(Cf.TINY_NET, 4, 4)
    assert m.vs_fp is False and m.unlabelled is False
    cfg = tmp_path / "vs.yaml"
    cfg.write_text("vs_fp: true\ntask: lits\n")
    args = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"]))
    assert args.vs_fp is True and args.unlabelled is False and args.task == "lits"
    cfg.write_text("unlabelled: true\n")
    args = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"]))
    assert args.unlabelled is True and args.vs_fp is False


def _parse(*flags):
    return Cf.build_parser().parse_args(["ptq", *flags])


@pytest.mark.parametrize("flags,named", [(("--unlabelled",), ("--unlabelled", "--vs_fp")),
                                         (("--unlabelled", "--vs_fp", "--test_fp"), ("--unlabelled", "--test_fp")),
                                         (("--unlabelled", "--vs_fp", "--lesion_table"),
                                          ("--unlabelled", "--lesion_table"))])
def test_check_switches_refuses_what_cannot_run_and_names_the_switches(flags, named):
    with pytest.raises(SystemExit) as e:
        entrance.check_switches(_parse(*flags))
    assert all(n in str(e.value) for n in named)


def test_check_switches_lets_the_rest_through_and_main_calls_it_first():
    for flags in ((), ("--vs_fp",), ("--vs_fp", "--test_fp", "--lesion_table"), ("--unlabelled", "--vs_fp"),
                  ("--unlabelled", "--vs_fp", "--is_cc", "--surf_dist", "--save_nii")):
        assert entrance.check_switches(_parse(*flags)) is None
    assert entrance.check_switches(Cf.make_args(Cf.TINY_NET, 4, 4)) is None
    # main refuses before it builds a network or opens a device: no --task is given, which get_model_cube would trip on
    with pytest.raises(SystemExit) as e:
        entrance.main(["ptq", "--unlabelled"])
    assert "--vs_fp" in str(e.value)


# ---- the symbol ---------------------------------------------------------------------------------------------------
def _ctype(decl):
    decl = decl.strip()
    if "*" in decl:
        return _lib._P
    if decl.startswith("long long"):
        return _lib._LL
    return {"int": _lib._I, "float": _lib._F, "size_t": _lib._SZ}[decl.split()[0]]


def test_agreement_symbol_in_header_and_lib_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint effq_seg_agreement\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m
    want = [_ctype(a) for a in m.group(1).split(",")]
    got_res, got = _lib.SIGNATURES["effq_seg_agreement"]
    assert got == want and got_res == _lib._I and len(got) == 14
    # the same decision arguments, in the same places, as the tallies
    t = re.search(r"\bint effq_seg_tallies\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert "int C, long long S, int mode, int fuse, float thresh" in " ".join(t.split())
    assert "int C, long long S, int mode, int fuse, float thresh" in " ".join(m.group(1).split())
    ws = re.search(r"#define EFFQ_SEG_AGREEMENT_WS_BYTES (.*)", code).group(1)
    ws = ws.replace("EFFQ_SEG_TALLIES_MAX_CLASSES", str(_lib.SEG_TALLIES_MAX_CLASSES))
    assert re.fullmatch(r"[\d\s()*+]+", ws) and eval(ws) == _lib.SEG_AGREEMENT_WS_BYTES
    assert "seg_agree.hip" in open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()


# ---- data without labels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["lits", "brats"])
def test_segvolumes_without_labels_never_opens_seg(tmp_path, task):
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), task, ["b", "a"], (5, 6, 7))
    shutil.rmtree(os.path.join(data_dir, "seg"))
    ds = D.SegVolumes(data_dir, ["a", "b"], D.MODALITIES[task], "npy", labels=False)
    img, lab = ds[1]
    assert lab.numel() == 0 and lab.dtype == torch.uint8
    assert np.array_equal(img.numpy(), arrays["b"][0])
    with pytest.raises(FileNotFoundError):
        D.SegVolumes(data_dir, ["a", "b"], D.MODALITIES[task], "npy")[0]
    args = Cf.make_args(Cf.TINY_NET if task == "lits" else dict(Cf.TINY_NET, task="brats", nMod=4, nClass=4,
                                                                multi_label="brats"), 4, 4,
                        data_dir=data_dir, split_dir=split_dir, access_type="npy", merge_type=None, patch_size=None,
                        vs_fp=True, unlabelled=True)
    cube = D.get_data_cube(args)
    assert cube.labelled is False
    for loader in (cube.trainseqloader, cube.valloader):       # both splits are read that way
        for image, label in loader:
            assert label.numel() == 0 and image.shape[0] == 1 and image.shape[2:] == (5, 6, 7)


def test_calibration_data_of_unlabelled_volumes(tmp_path):
    from efficientq_amd import calibrate as K
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), "lits", ["a", "b"], (8, 8, 8))
    shutil.rmtree(os.path.join(data_dir, "seg"))
    args = Cf.make_args(Cf.TINY_NET, 4, 4, data_dir=data_dir, split_dir=split_dir, access_type="npy", merge_type=None,
                        patch_size=None, vs_fp=True, unlabelled=True, lwq_batchsz=2, lwq_patchsz="4,4,4")
    data, label = K.get_calibration_data(args, D.get_data_cube(args))
    assert data.shape == (2, 1, 4, 4, 4) and label.numel() == 0
    assert torch.equal(data[0, 0], torch.from_numpy(arrays["a"][0][0, 2:6, 2:6, 2:6]))


# ---- agreement.csv ------------------------------------------------------------------------------------------------
def _results(unit=None, lesions=False):
    res = []
    for s, name in enumerate(("s1", "s2")):
        counts = torch.tensor([[50 + s, 3, 7, 940 - s], [0, 0, 10, 990]], dtype=torch.int64)
        v = {"counts": counts, "flips": 15, "flip_frac": 15 / 1000,
             "logit_rel_mse": torch.tensor([0.25, 1e-3], dtype=torch.float64),
             "logit_max": torch.tensor([3.5, 0.125], dtype=torch.float64),
             "prob_mae": torch.tensor([0.015625, 2e-5], dtype=torch.float64)}
        v.update(E.metrics_from_counts(counts))
        if lesions:
            v["lesions"] = torch.tensor([[2, 3, 0, 1], [1, 0, 1, 0]])
        if unit is not None:
            v["surface"] = torch.tensor([[2.0, 1.5, 0.5], [9.0, 9.0, 9.0]], dtype=torch.float64)
            if unit == "mm":
                v["surface_unit"] = "mm"
        res.append({"name": name, "vs_fp": v})
    return res


BASE = ["subject", "class", "dsc", "sens", "spec", "acc", "both", "q_only", "fp_only", "neither", "flip_frac_class",
        "logit_rel_mse", "logit_max", "prob_mae"]


def test_agreement_csv_has_one_row_per_subject_and_class_in_the_documented_order(tmp_path):
    path = str(tmp_path / "agreement.csv")
    E.write_agreement_csv(path, _results() + [{"name": "no_fp", "counts": torch.zeros(2, 4)}])
    rows = list(csv.reader(open(path)))
    assert rows[0] == BASE
    assert [(r[0], r[1]) for r in rows[1:]] == [("s1", "0"), ("s1", "1"), ("s2", "0"), ("s2", "1")]
    assert rows[1][6:10] == ["50", "3", "7", "940"] and rows[3][6:10] == ["51", "3", "7", "939"]
    assert rows[1][10] == "%.7g" % (10 / 1000) and rows[2][10] == "%.7g" % (10 / 1000)
    assert rows[1][11:] == ["0.25", "3.5", "0.015625"] and rows[2][11:] == ["0.001", "0.125", "2e-05"]
    dsc = (2 * 50 + 1e-6) / (53 + 57 + 1e-6)
    assert float(rows[1][2]) == pytest.approx(dsc, rel=1e-6)


def test_agreement_csv_lesion_and_surface_columns_follow_the_metrics_rule(tmp_path):
    path = str(tmp_path / "agreement.csv")
    E.write_agreement_csv(path, _results("voxel", lesions=True))
    rows = list(csv.reader(open(path)))
    assert rows[0] == BASE + list(E.LESION_COLUMNS) + list(E.SURFACE_COLUMNS)
    assert rows[1][14:] == ["2", "3", "0", "1", "2", "1.5", "0.5"]
    E.write_agreement_csv(path, _results("mm"))
    rows = list(csv.reader(open(path)))
    assert rows[0] == BASE + list(E.SURFACE_COLUMNS_MM) and rows[2][14:] == ["9", "9", "9"]
    mixed = _results("mm")
    del mixed[1]["vs_fp"]["surface_unit"]
    with pytest.raises(RuntimeError):
        E.write_agreement_csv(path, mixed)


def test_agreement_means():
    m = E.agreement_means(_results())
    assert m["flip_frac"] == pytest.approx(0.015) and m["prob_mae"].tolist() == [0.015625, 2e-5]
    assert m["dsc"].shape == (2,) and m["logit_rel_mse"].tolist() == [0.25, 1e-3]
