"""The ``score`` mission, host side (no GPU): parsing and refusals of --score_class / --score_tol and of the list, the grid
and value refusals, the class table, the arithmetic of the normalised surface Dice, the C-ABI rows of the new symbols, the
unchanged surface of HipOps, and the mission end to end over a numpy stand-in for its three device calls that is built on
the yardsticks of test_geometry_cpu (surfaces, distances in fp32) and on the component restatement of
test_seg_lesions_cpu, with scores.csv and summary.csv checked cell by cell against the formulas."""
import csv
import gzip
import math
import os
import re
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, entrance, evaluate as E, nifti, score
from efficientq_amd.hip_ops import HipOps
from tests.test_geometry_cpu import (pack_header, ref_edt_mm_lines, ref_surface_counts_mm, ref_surface_metrics_mm)
from tests.test_ops_layout_cpu import SURFACE
from tests.test_seg_lesions_cpu import lesion_counts
from tests.test_seg_surface_cpu import ref_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
AFFINE = np.array([[0.75, 0, 0, -30.0], [0, 1.5, 0, 12.0], [0, 0, 5.0, 4.0], [0, 0, 0, 1]], dtype=np.float64)
SPACING = (0.75, 1.5, 5.0)            # array axes 0, 1, 2
SHAPE = (10, 9, 6)


# ---- the yardstick of the device calls ---------------------------------------------------------------------------------
def tol_sq(t):
    return F32(np.float64(t) ** 2)


def ref_within(pred, gt, spacing, tols):
    """[[S(P) voxels with E_L <= T^2 per T], [S(L) voxels with E_P <= T^2 per T]] in fp32; none when the target is empty."""
    sp, sl = ref_surface(pred), ref_surface(gt)
    e_pl, e_lp = ref_edt_mm_lines(sl, spacing)[sp], ref_edt_mm_lines(sp, spacing)[sl]
    return [[int((e_pl <= tol_sq(t)).sum()) for t in tols], [int((e_lp <= tol_sq(t)).sum()) for t in tols]]


def class_masks(a, classes):
    return [np.isin(a, labels) for labels in classes]


def numpy_calls(classes):
    """The three device calls of score.run on the host, from the yardsticks (the table is checked against the classes)."""
    def masks(pred, truth, lut, C):
        assert pred.dtype == torch.uint8 and truth.dtype == torch.uint8 and pred.shape == truth.shape and C == len(classes)
        assert list(lut) == Cf.score_class_lut(classes)
        return class_masks(pred.numpy(), classes), class_masks(truth.numpy(), classes)

    def tallies(pred, truth, lut, C):
        p, t = masks(pred, truth, lut, C)
        return torch.tensor([[int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum()), int((~a & ~b).sum())]
                             for a, b in zip(p, t)], dtype=torch.int64)

    def lesions(pred, truth, lut, C):
        p, t = masks(pred, truth, lut, C)
        return torch.tensor([lesion_counts(a, b) for a, b in zip(p, t)], dtype=torch.int64)

    def surface(pred, truth, lut, C, spacing, tols=()):
        p, t = masks(pred, truth, lut, C)
        ref = [ref_surface_counts_mm(a, b, spacing) for a, b in zip(p, t)]
        within = torch.tensor([ref_within(a, b, spacing, tols) for a, b in zip(p, t)], dtype=torch.int64)
        return (torch.tensor([r[0] for r in ref], dtype=torch.int64),
                torch.tensor(np.array([r[1] for r in ref], F32)),
                torch.tensor([r[2] for r in ref], dtype=torch.float64), within.reshape(C, 2, len(tols)))
    return SimpleNamespace(tallies=tallies, lesions=lesions, surface=surface)


# ---- files ---------------------------------------------------------------------------------------------------------------
def blobs(seed, shape=SHAPE):
    """A label map of 0, 1, 2: a liver box with a tumour box inside and a speck of tumour elsewhere."""
    g = np.random.default_rng(seed)
    a = np.zeros(shape, np.uint8)
    lo = g.integers(1, 3, 3)
    a[lo[0]:lo[0] + 6, lo[1]:lo[1] + 5, lo[2]:lo[2] + 3] = 1
    a[lo[0] + 2:lo[0] + 4, lo[1] + 1:lo[1] + 3, lo[2] + 1:lo[2] + 2] = 2
    a[9, 8, int(g.integers(0, 6))] = 2
    return a


def write_float_image(path, a, affine=AFFINE):
    """A float32 NIfTI image packed by hand (nifti.write_nifti writes integers only)."""
    rows = [tuple(float(v) for v in affine[k]) for k in range(3)]
    raw = pack_header("<", a.shape, 16, 32, (1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0), 0, 1, (0.0,) * 6, rows)
    raw += np.asarray(a, dtype="<f4").tobytes(order="F")
    with gzip.open(path, "wb") as f:
        f.write(raw)


def write_pairs(root, maps, ct=True):
    """maps: {subject: (pred or None, truth or None)}; writes pred/<sn>.nii.gz, src/<sn>_seg.nii.gz and cases.csv."""
    for d in ("src", "pred"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    lines = []
    for sn, (pred, truth) in maps.items():
        nifti.write_nifti(os.path.join(root, "src", f"{sn}_ct.nii.gz"), np.zeros(SHAPE, np.uint8), AFFINE)
        cell = ""
        if truth is not None:
            cell = os.path.join("src", f"{sn}_seg.nii.gz")
            nifti.write_nifti(os.path.join(root, cell), truth, AFFINE)
        if pred is not None:
            nifti.write_nifti(os.path.join(root, "pred", f"{sn}.nii.gz"), pred, AFFINE)
        lines.append(f"{sn},src/{sn}_ct.nii.gz,{cell}\n")
    lst = os.path.join(root, "cases.csv")
    with open(lst, "w") as f:
        f.write("subject,ct,seg\n" + "".join(lines))
    return lst


def score_args(root, *extra, **over):
    a = Cf.build_parser().parse_args(["score", "--task", "lits", "--src_list", os.path.join(root, "cases.csv"),
                                      "--pred_dir", os.path.join(root, "pred"), "--out_dir", os.path.join(root, "score")]
                                     + list(extra))
    for k, v in over.items():
        setattr(a, k, v)
    return a


def refused(args, named, classes=Cf.SCORE_CLASSES["lits"]):
    with pytest.raises(SystemExit) as e:
        score.run(args, calls=numpy_calls(classes))
    assert all(n in str(e.value) for n in named), str(e.value)
    assert not os.path.exists(args.out_dir)


# ---- parsing ---------------------------------------------------------------------------------------------------------------
def test_parser_knows_the_mission_and_its_switches_and_yaml_sets_them(tmp_path):
    a = Cf.build_parser().parse_args(["score", "--task", "brats", "--score_class", "1,2,4", "--score_class", "4",
                                      "--score_tol", "3,1", "--pred_dir", "seg"])
    assert a.mission == "score" and a.pred_dir == "seg"
    assert Cf.score_switches(a) == (((1, 2, 4), (4,)), (1.0, 3.0))
    cfg = tmp_path / "s.yaml"
    cfg.write_text("score_class: ['1,2', [2]]\nscore_tol: [2, 0.5]\n")
    b = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["score", "--task", "lits"]))
    assert Cf.score_switches(b) == (((1, 2), (2,)), (0.5, 2.0))
    d = Cf.build_parser().parse_args(["score", "--task", "lits"])
    assert Cf.score_switches(d) == (((1, 2), (2,)), (1.0,))
    d.score_tol = "none"
    assert Cf.score_switches(d)[1] == ()
    d.score_tol = 2
    assert Cf.score_switches(d)[1] == (2.0,)
    assert Cf.score_switches(Cf.build_parser().parse_args(["score", "--task", "brats"]))[0] == ((1, 2, 4), (1, 4), (4,))


@pytest.mark.parametrize("value,named", [("0", "1 to 255"), ("256", "1 to 255"), ("1,x", "'x'"), ("1,,2", "''"),
                                         ("2,2", "twice"), ("-1", "1 to 255"), ("1.5", "1 to 255")])
def test_score_class_values_that_are_not_understood_are_refused_by_name(value, named):
    a = Cf.build_parser().parse_args(["score", "--task", "lits"])
    a.score_class = [value]
    with pytest.raises(SystemExit) as e:
        Cf.score_switches(a)
    assert "--score_class" in str(e.value) and named in str(e.value)


def test_more_than_eight_classes_or_tolerances_and_an_unknown_task_are_refused():
    a = Cf.build_parser().parse_args(["score", "--task", "lits"])
    a.score_class = [str(v) for v in range(1, 10)]
    with pytest.raises(SystemExit, match="at most 8"):
        Cf.score_switches(a)
    a.score_class, a.score_tol = None, ",".join(str(v) for v in range(9))
    with pytest.raises(SystemExit, match="1 to 8"):
        Cf.score_switches(a)
    a.score_tol, a.task = None, "kits"
    with pytest.raises(SystemExit, match="--task"):
        Cf.score_switches(a)
    a.score_class = ["1"]                   # with classes of its own any task name will do
    assert Cf.score_switches(a) == (((1,),), (1.0,))


@pytest.mark.parametrize("value,named", [("-1", ">= 0"), ("nan", "finite"), ("inf", "finite"), ("1,1", "twice"),
                                         ("1,1.0", "twice"), ("a", "no number"), ("", "no number"), ("1,,2", "no number"),
                                         ("1,1.00000001", "print alike")])
def test_score_tol_values_that_are_not_understood_are_refused_by_name(value, named):
    a = Cf.build_parser().parse_args(["score", "--task", "lits"])
    a.score_tol = value
    with pytest.raises(SystemExit) as e:
        Cf.score_switches(a)
    assert "--score_tol" in str(e.value) and named in str(e.value)


FOREIGN = [["--post", "1:largest"], ["--thresh", "0.4"], ["--thr_sweep"], ["--save_prob"], ["--save_unc"],
           ["--lesion_match"], ["--lesion_table"], ["--blend", "gauss"], ["--tta_mirror", "w"], ["--resume", "x.pkl"],
           ["--pretrain", "x.pkl"], ["--prep_mask", "all"], ["--prep_window", "-200,250"], ["--prep_orient", "RAS"],
           ["--prep_spacing", "1,1,1"], ["--prep_antialias"], ["--prep_interp", "cubic"], ["--prep_min_size", "8,8,8"],
           ["--prep_no_crop"]]


@pytest.mark.parametrize("switch", FOREIGN, ids=[s[0] for s in FOREIGN])
def test_every_foreign_switch_is_refused_by_name_in_score(tmp_path, switch):
    root = str(tmp_path)
    write_pairs(root, {"a": (blobs(1), blobs(2))})
    with pytest.raises(SystemExit) as e:
        entrance.main(["score", "--task", "lits", "--src_list", os.path.join(root, "cases.csv"), "--pred_dir",
                       os.path.join(root, "pred"), "--out_dir", os.path.join(root, "score")] + switch)
    assert switch[0] in str(e.value) and "score mission" in str(e.value), str(e.value)
    assert not os.path.exists(os.path.join(root, "score"))
    assert {s for s, _ in Cf.SCORE_FOREIGN} == {s[0][2:] for s in FOREIGN}


@pytest.mark.parametrize("mission", ["ptq", "prep", "predict"])
@pytest.mark.parametrize("switch", [["--pred_dir", "seg"], ["--score_class", "1"], ["--score_tol", "1"]],
                         ids=["pred_dir", "score_class", "score_tol"])
def test_the_score_switches_are_refused_by_name_in_the_other_missions(mission, switch):
    with pytest.raises(SystemExit) as e:
        entrance.main([mission, "--task", "lits"] + switch)
    assert switch[0] in str(e.value) and f"the {mission} mission" in str(e.value), str(e.value)
    assert Cf.score_switches(Cf.build_parser().parse_args([mission, "--task", "lits"])) is None


# ---- the list, the grids and the values ------------------------------------------------------------------------------------
def test_refusals_of_the_list_name_their_cause_and_leave_out_dir_alone(tmp_path):
    root = str(tmp_path)
    a, b = blobs(1), blobs(2)
    write_pairs(root, {"a": (a, b), "b": (None, b), "c": (a, None)})
    refused(score_args(root), ["--pred_dir", "subject b", "b.nii.gz"])
    with open(os.path.join(root, "noseg.csv"), "w") as f:
        f.write("subject,ct\na,src/a_ct.nii.gz\n")
    refused(score_args(root, src_list=os.path.join(root, "noseg.csv")), ["noseg.csv", "no seg column"])
    with open(os.path.join(root, "nobody.csv"), "w") as f:
        f.write("subject,ct,seg\na,src/a_ct.nii.gz,\nc,src/c_ct.nii.gz,\n")
    refused(score_args(root, src_list=os.path.join(root, "nobody.csv")), ["nobody.csv", "no subject has a seg cell"])
    refused(score_args(root, pred_dir=None), ["--pred_dir"])
    refused(score_args(root, task="kits"), ["--task"])
    # an uncompressed map is found too
    nifti.write_nifti(os.path.join(root, "pred", "b.nii"), a, AFFINE)
    rows = score.run(score_args(root), calls=numpy_calls(Cf.SCORE_CLASSES["lits"]))
    assert [r["subject"] for r in rows] == ["a", "a", "b", "b"]


def test_grid_refusals_name_the_subject_before_anything_is_scored(tmp_path):
    root = str(tmp_path)
    a, b = blobs(1), blobs(2)
    write_pairs(root, {"a": (a, b), "b": (a, b)})
    pred_b = os.path.join(root, "pred", "b.nii.gz")
    nifti.write_nifti(pred_b, np.zeros((10, 9, 7), np.uint8), AFFINE)
    refused(score_args(root), ["subject b", "shape", "(10, 9, 7)"])
    moved = AFFINE.copy()
    moved[0, 3] += 0.5
    nifti.write_nifti(pred_b, a, moved)
    refused(score_args(root), ["subject b", "affine", "translation"])
    scaled = AFFINE.copy()
    scaled[2, 2] = 4.0
    nifti.write_nifti(pred_b, a, scaled)
    refused(score_args(root), ["subject b", "affine", "3 x 3"])
    # 2 C planes past the limits of the device calls: a header alone says so
    big = os.path.join(root, "src", "b_seg.nii.gz")
    rows3 = [tuple(float(v) for v in AFFINE[k]) for k in range(3)]
    for path in (pred_b, big):
        with gzip.open(path, "wb") as f:
            f.write(pack_header("<", (4097, 2, 2), 2, 8, (1.0,) * 4 + (0,) * 4, 0, 1, (0.0,) * 6, rows3))
    refused(score_args(root), ["subject b", "limits", "4096"])


@pytest.mark.parametrize("kind,said", [("half", "2.5"), ("big", "300"), ("nan", "nan"), ("negative", "-1")])
@pytest.mark.parametrize("which", ["pred", "seg"])
def test_value_refusals_name_subject_file_and_value(tmp_path, kind, said, which):
    root = str(tmp_path)
    a, b = blobs(1), blobs(2)
    write_pairs(root, {"a": (a, b), "b": (a, b)})
    path = os.path.join(root, "pred", "b.nii.gz") if which == "pred" else os.path.join(root, "src", "b_seg.nii.gz")
    if kind == "half":                  # scl_slope applies: stored 2 a reads a, stored 5 reads 2.5
        stored = 2 * a
        stored[3, 4, 2] = 5
        nifti.write_nifti(path, stored, AFFINE, scale=(0.5, 0.0))
    elif kind == "big":
        wide = a.astype(np.uint16)
        wide[3, 4, 2] = 300
        nifti.write_nifti(path, wide, AFFINE)
    else:
        f = a.astype(np.float32)
        f[3, 4, 2] = np.nan if kind == "nan" else -1.0
        write_float_image(path, f)
    args = score_args(root)
    with pytest.raises(SystemExit) as e:
        score.run(args, calls=numpy_calls(Cf.SCORE_CLASSES["lits"]))
    msg = str(e.value)
    assert "subject b" in msg and path in msg and f"value {said}" in msg and "3 4 2" in msg, msg
    assert not os.path.exists(os.path.join(args.out_dir, score.SCORES_CSV))


def test_a_float_image_of_whole_numbers_and_a_scaled_one_are_label_maps(tmp_path):
    a = blobs(3)
    path = str(tmp_path / "f.nii.gz")
    write_float_image(path, a.astype(np.float32))
    assert np.array_equal(score.read_labels("s", path), a)
    nifti.write_nifti(path, a, AFFINE, scale=(2.0, 1.0))
    assert np.array_equal(score.read_labels("s", path), 2 * a + 1)


# ---- classes and the arithmetic ----------------------------------------------------------------------------------------------
def test_class_table_of_the_brats_default_is_post_class_luts():
    assert Cf.score_class_lut(Cf.SCORE_CLASSES["brats"]) == E.post_class_lut("brats", 3)
    assert Cf.score_class_lut(((1,), (2,))) == [0, 1, 2] + [0] * 253
    lits = Cf.score_class_lut(Cf.SCORE_CLASSES["lits"])
    assert lits[:3] == [0, 0b01, 0b11] and not any(lits[3:])


def test_nsd_arithmetic_and_its_empty_rules():
    assert score.nsd(0, 0, 0, 0) == 1.0
    assert score.nsd(0, 0, 5, 0) == 0.0 and score.nsd(0, 0, 0, 7) == 0.0
    assert score.nsd(3, 4, 5, 9) == 0.5 and score.nsd(5, 9, 5, 9) == 1.0 and score.nsd(0, 0, 5, 9) == 0.0
    assert score.nsd_column(1.0) == "nsd_1mm" and score.nsd_column(0.5) == "nsd_0.5mm" and score.nsd_column(0) == "nsd_0mm"
    assert score.lesion_rates(4, 5, 1, 2) == (0.75, 0.6) and score.lesion_rates(0, 0, 0, 0) == (1.0, 1.0)
    assert score.lesion_rates(0, 3, 0, 3) == (1.0, 0.0)


def test_tolerances_are_squared_as_the_axis_weights_are():
    from efficientq_amd import ops_score
    assert ops_score.tolerances_sq("t", (0, 0.7421875, 3)) == [0.0, float(tol_sq(0.7421875)), 9.0]
    assert ops_score.tolerances_sq("t", ()) == []
    for bad in ((-1,), (float("nan"),), (float("inf"),), (2, 1), (1, 1), tuple(range(9)), (1e30,), "ab", (1, 1 + 1e-12)):
        with pytest.raises(_lib.EffqError, match="tols"):
            ops_score.tolerances_sq("t", bad)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_score_symbols_in_header_signatures_and_makefile():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("effq_label_lesions", 12), ("effq_label_surface_mm_ws_bytes", 5), ("effq_label_surface_mm", 19)):
        m = re.search(rf"\b(?:int|size_t) {name}\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"\bsize_t effq_label_surface_mm_ws_bytes\s*\(\s*int C, int D, int H, int W, int ntol\s*\)", hdr)
    assert int(re.search(r"#define EFFQ_SURF_TOL_MAX (\d+)", hdr).group(1)) == _lib.SURF_TOL_MAX == Cf.SCORE_MAX_TOLS == 8
    floats = [i for i, t in enumerate(_lib.SIGNATURES["effq_label_surface_mm"][1]) if t is _lib._F]
    assert floats == [7, 8, 9]
    csrc = os.path.join(ROOT, "efficientq_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert srcs.count("label_score.hip") == 1 and "label_bits.h" in re.search(r"^%\.o:(.*)$", mk, re.M).group(1).split()
    text = open(os.path.join(csrc, "label_score.hip")).read()
    assert re.search(r"^int effq_label_lesions\s*\(", text, re.M) and '#include "label_bits.h"' in text
    assert "cc_run(cc_src_bits(" in text
    bits = open(os.path.join(csrc, "label_bits.h")).read()
    assert "void k_label_bits" in bits and "__shared__ uint16_t s_lut[256]" in bits and "ushort4" in bits
    mm = open(os.path.join(csrc, "seg_surface_mm.hip")).read()
    assert "void k_surf_within" in mm and re.search(r"^int effq_label_surface_mm\s*\(", mm, re.M)
    # both entry points of the surface distances run one launch sequence after their bits
    assert mm.count("mm_surface_run(s, C, D, H, W, wd, wh, ww, counts, sq, sums, st)") == 2
    lib = _lib.load()
    assert lib.effq_label_surface_mm_ws_bytes(3, 5, 6, 7, 2) == \
        (lib.effq_surf_mm_ws_bytes(6, 5, 6, 7) + 15) // 16 * 16 + 1152
    for bad in ((0, 5, 6, 7, 1), (9, 5, 6, 7, 1), (3, 5, 6, 7, 9), (3, 5, 6, 7, -1), (3, 4097, 1, 1, 1), (3, 0, 6, 7, 1)):
        assert lib.effq_label_surface_mm_ws_bytes(*bad) == 0, bad


def test_host_side_argument_checks_launch_nothing_without_a_device():
    """Every check of the two entry points runs before the first launch, so a host without a device can ask for them."""
    import ctypes as C
    lib = _lib.load()
    lut = (C.c_uint16 * 256)(*Cf.score_class_lut(Cf.SCORE_CLASSES["lits"]))
    bad_lut = (C.c_uint16 * 256)(*([0] * 255 + [4]))
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    ARG = 1
    assert lib.effq_label_lesions(p, p, 2, 2, 2, 2, bad_lut, 26, p, p, 1 << 20, None) == ARG
    assert lib.effq_label_lesions(p, p, 2, 2, 2, 2, lut, 18, p, p, 1 << 20, None) == ARG
    assert lib.effq_label_lesions(p, None, 2, 2, 2, 2, lut, 26, p, p, 1 << 20, None) == ARG
    assert lib.effq_label_lesions(p, p, 2, 2, 2, 2, lut, 26, p, p, 16, None) == 3          # EFFQ_ERR_WORKSPACE

    def surf(tols, lut_=lut, n=None, within=p, nbytes=1 << 20):
        t = (C.c_float * max(len(tols), 1))(*tols)
        return lib.effq_label_surface_mm(p, p, 2, 2, 2, 2, lut_, 1.0, 1.0, 1.0, t, len(tols) if n is None else n, p, p, p,
                                         within, p, nbytes, None)
    for tols in ([-1.0], [float("nan")], [float("inf")], [2.0, 1.0], [1.0, 1.0], [0.0] * 9):
        assert surf(tols) == ARG, tols
    assert surf([1.0], lut_=bad_lut) == ARG and surf([1.0], within=None) == ARG and surf([1.0], n=-1) == ARG
    assert surf([1.0], nbytes=lib.effq_label_surface_mm_ws_bytes(2, 2, 2, 2, 1) - 1) == ARG
    assert not any(buf)


def test_the_surface_of_hip_ops_is_unchanged():
    names = [n for n in dir(HipOps) if not n.startswith("__")]
    assert names == [n for n, _ in SURFACE]
    assert not any("label_lesions" in n or "label_surface" in n for n in names)


# ---- the whole mission on the host -------------------------------------------------------------------------------------------
def f32_ratios(tp, fp, fn, tn):
    """metrics.py:21-45 in numpy fp32 on the integer sums."""
    eps = F32(1e-6)
    tp_, fp_, fn_, tn_ = (F32(v) for v in (tp, fp, fn, tn))
    return [(F32(2 * tp) + eps) / (F32(tp + fp) + F32(tp + fn) + eps), (tp_ + eps) / (F32(tp + fn) + eps),
            (tn_ + eps) / (F32(tn + fp) + eps), F32(tp + tn) / F32(tp + fp + fn + tn)]


def g7(v):
    return "%.7g" % float(v)


@pytest.mark.parametrize("task_classes,tols_arg,tols", [(None, "3,1", (1.0, 3.0)), (("1,2", "2", "1"), "none", ()),
                                                        (None, None, (1.0,))])
def test_whole_mission_writes_scores_and_summary_that_the_formulas_reproduce(tmp_path, capsys, task_classes, tols_arg,
                                                                              tols):
    root = str(tmp_path)
    a_pred, a_true = blobs(1), blobs(2)
    b_pred, b_true = blobs(3), blobs(4)
    b_pred[b_pred == 2] = 1                                  # no tumour predicted: one surface of class 1 is empty
    e_pred = np.where(blobs(5) == 2, 0, blobs(5)).astype(np.uint8)
    e_true = np.where(blobs(6) == 2, 0, blobs(6)).astype(np.uint8)   # no tumour at all: both surfaces of class 1 are empty
    write_pairs(root, {"b": (b_pred, b_true), "a": (a_pred, a_true), "u": (a_pred, None), "e": (e_pred, e_true)})
    extra = [] if task_classes is None else [w for c in task_classes for w in ("--score_class", c)]
    extra += [] if tols_arg is None else ["--score_tol", tols_arg]
    args = score_args(root, *extra)
    classes = Cf.SCORE_CLASSES["lits"] if task_classes is None else tuple(Cf.parse_score_class(c) for c in task_classes)
    rows = score.run(args, calls=numpy_calls(classes))
    said = capsys.readouterr().out
    assert "1 subjects without a seg cell are skipped: u" in said
    assert all(f"[score] {sn}:" in said for sn in "abe") and "[score] u:" not in said
    assert all(f"[score] class {c} " in said for c in range(len(classes)))
    got = list(csv.reader(open(os.path.join(args.out_dir, "scores.csv"))))
    cols = ["subject", "class", "labels", "dsc", "sens", "spec", "acc", "tp", "fp", "fn", "tn", "pred_ml", "label_ml",
            "totall", "predl", "fnl", "fpl", "hd_mm", "hd95_mm", "assd_mm"] + ["nsd_%gmm" % t for t in tols]
    assert got[0] == cols and len(got) == 1 + 3 * len(classes) == 1 + len(rows)
    ml = 0.75 * 1.5 * 5.0 / 1000.0
    want_rows = []
    for sn, pred, truth in (("a", a_pred, a_true), ("b", b_pred, b_true), ("e", e_pred, e_true)):
        for c, labels in enumerate(classes):
            p, t = np.isin(pred, labels), np.isin(truth, labels)
            tp, fp, fn, tn = int((p & t).sum()), int((p & ~t).sum()), int((~p & t).sum()), int((~p & ~t).sum())
            n_p, n_l = int(ref_surface(p).sum()), int(ref_surface(t).sum())
            within = ref_within(p, t, SPACING, tols)
            nsds = [1.0 if n_p == n_l == 0 else 0.0 if 0 in (n_p, n_l) else (within[0][k] + within[1][k]) / (n_p + n_l)
                    for k in range(len(tols))]
            want_rows.append(dict(sn=sn, c=c, ratios=f32_ratios(tp, fp, fn, tn), counts=[tp, fp, fn, tn],
                                  ml=[(tp + fp) * ml, (tp + fn) * ml], lesions=lesion_counts(p, t),
                                  surf=ref_surface_metrics_mm(p, t, SPACING), nsd=nsds, empty=(n_p == 0, n_l == 0)))
    for line, w in zip(got[1:], want_rows):
        want = [w["sn"], str(w["c"]), " ".join(str(v) for v in classes[w["c"]])] + [g7(v) for v in w["ratios"]] + \
            [str(v) for v in w["counts"]] + [g7(v) for v in w["ml"]] + [str(v) for v in w["lesions"]] + \
            [g7(v) for v in w["surf"]] + [g7(v) for v in w["nsd"]]
        assert line == want, (line, want)
    # the cases are what they were built to be
    by = {(w["sn"], w["c"]): w for w in want_rows}
    assert by[("b", 1)]["empty"] == (True, False) and by[("e", 1)]["empty"] == (True, True)
    diag = math.sqrt(sum((n * s) ** 2 for n, s in zip(SHAPE, SPACING)))
    assert by[("b", 1)]["surf"] == (diag,) * 3 and by[("e", 1)]["surf"] == (0.0,) * 3
    if tols:
        assert by[("b", 1)]["nsd"] == [0.0] * len(tols) and by[("e", 1)]["nsd"] == [1.0] * len(tols)
        assert 0.0 < by[("a", 0)]["nsd"][0] < 1.0
    if len(tols) == 2:
        assert by[("a", 0)]["nsd"][0] < by[("a", 0)]["nsd"][1]
    summ = list(csv.reader(open(os.path.join(args.out_dir, "summary.csv"))))
    assert summ[0] == ["class", "labels", "cases", "dsc", "hd95_mm", "assd_mm"] + ["nsd_%gmm" % t for t in tols] + \
        ["totall", "predl", "fnl", "fpl", "lesion_sens", "lesion_prec"]
    assert len(summ) == 1 + len(classes)
    for c, line in enumerate(summ[1:]):
        mine = [w for w in want_rows if w["c"] == c]
        les = [sum(w["lesions"][k] for w in mine) for k in range(4)]
        means = [sum(float(w["ratios"][0]) for w in mine) / 3, sum(w["surf"][1] for w in mine) / 3,
                 sum(w["surf"][2] for w in mine) / 3] + [sum(w["nsd"][k] for w in mine) / 3 for k in range(len(tols))]
        want = [str(c), " ".join(str(v) for v in classes[c]), "3"] + [g7(v) for v in means] + [str(v) for v in les] + \
            [g7(1 - les[2] / les[0] if les[0] else 1.0), g7(1 - les[3] / les[1] if les[1] else 1.0)]
        assert line == want, (line, want)
    assert sorted(os.listdir(args.out_dir)) == ["scores.csv", "summary.csv"]
