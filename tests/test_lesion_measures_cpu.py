"""``--lesion_measures``, host side (no GPU): the line-end argument of the diameter search bit for bit against the brute
force over all voxel pairs, the switches and every refusal by name, the slice axis from the header, the C-ABI row of the
new symbol, and the score and predict missions end to end over the yardstick of tests/lesion_measure_ref.py injected for
the device call, with lesions.csv and lesion_detect.csv checked cell by cell and every other file byte for byte."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, entrance, lesion_measures as LM, nifti, predict, prep, score
from efficientq_amd.prep import PrepError
from tests import lesion_measure_ref as R
from tests.test_post_cpu import PostOps
from tests.test_predict_cpu import PointNet, PredictOps, predict_args, write_cases
from tests.test_prep_cpu import written
from tests.test_score_cpu import numpy_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITS = Cf.SCORE_CLASSES["lits"]
# array axis 0 runs towards -z at 2.5 mm, axis 1 towards +x at 0.7, axis 2 towards -y at 0.8: the slice axis is 0
FLIPPED = np.array([[0, 0.7, 0, -10.0], [0, 0, -0.8, 33.0], [-2.5, 0, 0, 50.0], [0, 0, 0, 1.0]])
PLAIN = np.array([[0.75, 0, 0, -30.0], [0, 1.5, 0, 12.0], [0, 0, 5.0, 4.0], [0, 0, 0, 1.0]])


# ---- line ends against all pairs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("spacing", R.SPACINGS)
def test_the_greatest_energy_over_line_ends_has_the_bits_of_the_one_over_all_voxel_pairs(conn, spacing):
    g = np.random.default_rng(7 * conn + int(100 * spacing[2]))
    w = R.weights(spacing)
    seen = 0
    for trial in range(6):
        shape = tuple(int(v) for v in g.integers(4, 14, 3))
        mask = g.random(shape) < (0.25, 0.45, 0.7)[trial % 3]
        lab, n = R.components(mask, conn)
        for k in range(1, n + 1):
            comp = lab == k
            if comp.sum() < 3:
                continue
            seen += 1
            for axis in (0, 1, 2):
                brute, lines = R.farthest_brute(comp, w, axis), R.farthest_lines(comp, w, axis)
                for kind in (0, 1):
                    assert np.array(brute[kind][0]).view(np.uint32) == np.array(lines[kind][0]).view(np.uint32)
                    # the pair of the lines is one of the voxels, attains that E and, for kind 1, lies in one slice
                    e, a, b = lines[kind]
                    assert a <= b and comp.ravel()[a] and comp.ravel()[b]
                    assert R.pair_bits(a, b, shape, w) == int(np.array(e).view(np.uint32))
                    if kind:
                        assert np.unravel_index(a, shape)[axis] == np.unravel_index(b, shape)[axis]
    assert seen >= 6


def test_a_one_voxel_component_is_its_own_pair_at_energy_zero():
    comp = np.zeros((3, 4, 5), bool)
    comp[1, 2, 3] = True
    v = int(np.ravel_multi_index((1, 2, 3), comp.shape))
    for far in (R.farthest_brute, R.farthest_lines):
        assert far(comp, R.weights((0.7, 0.7, 2.5)), 0) == [(0.0, v, v), (0.0, v, v)]


# ---- the switches ---------------------------------------------------------------------------------------------------------
def parse(mission, *extra):
    return Cf.build_parser().parse_args([mission, "--task", "lits"] + list(extra))


def test_parser_knows_the_switches_and_yaml_sets_them(tmp_path):
    a = parse("predict", "--lesion_measures", "--measure_class", "1,2", "--measure_class", "2", "--measure_plane", "h")
    assert a.lesion_measures is True and a.measure_class == ["1,2", "2"] and a.measure_plane == "h"
    assert Cf.measure_switches(a) == (((1, 2), (2,)), "h")
    b = parse("score")
    assert b.lesion_measures is False and b.measure_class is None and b.measure_plane is None
    assert Cf.measure_switches(b) is None
    assert Cf.measure_switches(parse("score", "--lesion_measures")) == (None, "axial")
    y = tmp_path / "m.yaml"
    y.write_text("lesion_measures: true\nmeasure_class: [[1, 2], 2]\nmeasure_plane: w\n")
    c = Cf.merge_config(str(y), parse("predict"))
    assert Cf.measure_switches(c) == (((1, 2), (2,)), "w")


@pytest.mark.parametrize("mission", ["ptq", "prep"])
@pytest.mark.parametrize("switch,extra", [("lesion_measures", ["--lesion_measures"]),
                                          ("measure_class", ["--measure_class", "1"]),
                                          ("measure_plane", ["--measure_plane", "d"])])
def test_ptq_and_prep_refuse_the_three_switches_by_name(tmp_path, monkeypatch, mission, switch, extra):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        Cf.measure_switches(parse(mission, *extra))
    assert f"--{switch}" in str(e.value) and mission in str(e.value)
    argv = [mission, "--task", "lits"] + extra + (["--synthetic"] if mission == "ptq" else ["--src_list", "none.csv"])
    with pytest.raises(SystemExit) as e:
        entrance.main(argv)
    assert f"--{switch}" in str(e.value)
    assert os.listdir(str(tmp_path)) == []


def test_values_and_combinations_that_cannot_be_served_are_refused_by_name():
    def refused(args, *named):
        with pytest.raises(SystemExit) as e:
            Cf.measure_switches(args)
        assert all(n in str(e.value) for n in named), str(e.value)
    refused(parse("score", "--lesion_measures", "--measure_class", "1"), "--measure_class", "--score_class")
    refused(parse("score", "--measure_class", "1"), "--measure_class")
    refused(parse("predict", "--measure_class", "1"), "--measure_class", "--lesion_measures")
    refused(parse("predict", "--measure_plane", "d"), "--measure_plane", "--lesion_measures")
    refused(parse("score", "--measure_plane", "axial"), "--measure_plane", "--lesion_measures")
    refused(parse("predict", "--lesion_measures", "--measure_plane", "z"), "--measure_plane", "'z'", "axial")
    refused(parse("predict", "--lesion_measures", "--measure_class", "0"), "--measure_class", "'0'")
    refused(parse("predict", "--lesion_measures", "--measure_class", "3,3"), "--measure_class", "twice")
    nine = [s for k in range(1, 10) for s in ("--measure_class", str(k))]
    refused(parse("predict", "--lesion_measures", *nine), "--measure_class", "9 classes")
    assert Cf.SCORE_FOREIGN[5:7] == (("lesion_match", False), ("lesion_table", False))      # it stays what it is


# ---- the slice axis ---------------------------------------------------------------------------------------------------------
def test_axial_is_the_array_axis_nearest_to_world_z_also_when_permuted_and_flipped():
    for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 2, 1)):
        for flips in ((1, 1, 1), (-1, 1, -1), (1, -1, -1)):
            A = np.eye(4)
            A[:3, :3] = 0.0
            for a in range(3):
                A[perm[a], a] = flips[a] * (0.7, 1.3, 2.5)[a]
            A[:3, :3] += 0.01 * np.array([[0, 1, -1], [1, 0, 1], [-1, 1, 0]])       # a little oblique
            assert LM.slice_axis("axial", A, "s") == perm.index(2)
            assert [LM.slice_axis(p, A, "s") for p in "dhw"] == [0, 1, 2]
    assert LM.slice_axis("axial", FLIPPED, "s") == 0 and LM.slice_axis("axial", PLAIN, "s") == 2


def oblique():
    A = PLAIN.copy()
    A[:3, 2] = (0.0, 5.0 * np.sqrt(0.5), 5.0 * np.sqrt(0.5))         # array axis 2 at 45 degrees between y and z
    A[:3, 2] = (0.0, 3.0, 3.0)
    return A


def test_an_affine_at_45_degrees_is_refused_naming_the_subject_and_the_way_out():
    with pytest.raises(PrepError) as e:
        LM.slice_axis("axial", oblique(), "case7")
    assert all(n in str(e.value) for n in ("subject case7", "45 degrees", "--measure_plane d|h|w"))
    assert LM.slice_axis("w", oblique(), "case7") == 2


# ---- the symbol ---------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_in_the_header_the_signatures_and_the_makefile():
    with open(os.path.join(ROOT, "include", "effq_hip.h")) as f:
        hdr = f.read()
    for name, nargs in (("effq_label_lesion_measures_ws_bytes", 6), ("effq_label_lesion_measures", 20)):
        m = re.search(rf"\b{name}\(([^;]*?)\);", hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["effq_label_lesion_measures_ws_bytes"][0] is _lib._SZ
    floats = [i for i, t in enumerate(_lib.SIGNATURES["effq_label_lesion_measures"][1]) if t is _lib._F]
    assert floats == [8, 9, 10]
    assert int(re.search(r"#define EFFQ_LESION_MEASURE_WORDS (\d+)", hdr).group(1)) == _lib.LESION_MEASURE_WORDS == R.WORDS
    with open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")) as f:
        assert "label_measure.hip" in re.search(r"^SRCS\s*=(.*)$", f.read(), re.M).group(1).split()


# ---- the score mission -------------------------------------------------------------------------------------------------------
def two_maps(seed, shape):
    """A label map and a predicted map of 0, 1, 2: liver boxes with tumours, some found, one missed, one invented."""
    g = np.random.default_rng(seed)
    truth = np.zeros(shape, np.uint8)
    truth[1:shape[0] - 1, 1:shape[1] - 2, 1:shape[2] - 1] = 1
    truth[2:4, 2:4, 2:5] = 2
    truth[shape[0] - 3, shape[1] - 4, 1:3] = 2
    truth[0, shape[1] - 1, shape[2] - 1] = 2                          # a one-voxel lesion outside the liver
    pred = truth.copy()
    pred[shape[0] - 3, shape[1] - 4, 1:3] = 1                         # missed
    pred[2, 2, 2] = 1
    pred[1, shape[1] - 3, shape[2] - 3:shape[2] - 1] = 2              # invented
    pred[g.integers(0, shape[0]), 0, 0] = 1
    return pred, truth


def write_score_cases(root, cases):
    """cases: {subject: (pred, truth, affine)}; the layout of the score mission's list."""
    for d in ("src", "pred"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    lines = []
    for sn, (pred, truth, affine) in cases.items():
        nifti.write_nifti(os.path.join(root, "src", f"{sn}_ct.nii.gz"), np.zeros(pred.shape, np.uint8), affine)
        nifti.write_nifti(os.path.join(root, "src", f"{sn}_seg.nii.gz"), truth, affine)
        nifti.write_nifti(os.path.join(root, "pred", f"{sn}.nii.gz"), pred, affine)
        lines.append(f"{sn},src/{sn}_ct.nii.gz,src/{sn}_seg.nii.gz\n")
    with open(os.path.join(root, "cases.csv"), "w") as f:
        f.write("subject,ct,seg\n" + "".join(lines))


def score_args(root, out, *extra):
    return Cf.build_parser().parse_args(["score", "--task", "lits", "--src_list", os.path.join(root, "cases.csv"),
                                         "--pred_dir", os.path.join(root, "pred"), "--out_dir", os.path.join(root, out)]
                                        + list(extra))


def calls_with_measures(classes, seen):
    """tests.test_score_cpu.numpy_calls and the yardstick's arrays for the fourth call."""
    calls = numpy_calls(classes)

    def measures(pred, truth, lut, C, spacing, slice_axis):
        assert list(lut) == Cf.score_class_lut(classes) and C == len(classes)
        p, t = pred.numpy(), None if truth is None else truth.numpy()
        nrows, rows, meas, _ = R.measures(p, t, classes, 26, spacing, slice_axis)
        seen.append((tuple(float(s) for s in spacing), slice_axis))
        return None, torch.from_numpy(nrows), [torch.from_numpy(r) for r in rows], [torch.from_numpy(m) for m in meas]
    calls.measures = measures
    return calls


def cells(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_score_writes_the_two_tables_of_the_yardstick_and_leaves_the_others_byte_for_byte(tmp_path, capsys):
    root = str(tmp_path)
    cases = {"b": two_maps(1, (7, 9, 8)) + (FLIPPED,), "a": two_maps(2, (8, 8, 10)) + (PLAIN,)}
    write_score_cases(root, cases)
    seen = []
    score.run(score_args(root, "plain"), calls=numpy_calls(LITS))
    score.run(score_args(root, "with", "--lesion_measures"), calls=calls_with_measures(LITS, seen))
    said = capsys.readouterr().out
    assert written(os.path.join(root, "plain")) == ["scores.csv", "summary.csv"]
    assert written(os.path.join(root, "with")) == ["lesion_detect.csv", "lesions.csv", "scores.csv", "summary.csv"]
    for name in ("scores.csv", "summary.csv"):
        assert read(os.path.join(root, "plain", name)) == read(os.path.join(root, "with", name))
    # the spacing is the header's and the slice axis the one nearest to world z
    assert [s[1] for s in seen] == [2, 0] and seen[0][0] == (0.75, 1.5, 5.0)
    assert seen[1][0] == pytest.approx((2.5, 0.7, 0.8), rel=1e-7)           # the header holds fp32 rows
    want, diams = [], []
    for sn, axis in (("a", 2), ("b", 0)):
        pred, truth, _ = cases[sn]
        head = nifti.read_geometry(os.path.join(root, "pred", f"{sn}.nii.gz"))
        affine, spacing = np.asarray(head["affine"], np.float64), tuple(float(v) for v in head["spacing"])
        assert spacing == seen[("a", "b").index(sn)][0]
        _, rows, meas, _ = R.measures(pred, truth, LITS, 26, spacing, axis)
        c, d = R.expected_lesions(sn, LITS, True, rows, meas, pred.shape, spacing, affine, axis)
        want, diams = want + c, diams + d
    got = cells(os.path.join(root, "with", "lesions.csv"))
    assert got[0] == list(R.COLUMNS) == list(LM.LESION_COLUMNS)
    assert got[1:] == want and len(want) > 12
    kinds = [(r[0], r[1], r[3]) for r in want]
    assert kinds == sorted(kinds, key=lambda k: (k[0], k[1], k[2] != "label"))          # label lesions first
    assert {r[22] for r in want if r[0] == "b"} == {"d"} and {r[22] for r in want if r[0] == "a"} == {"w"}
    one = [r for r in want if r[8] == "1"]
    assert one and all(r[19] == "0" and r[20] == r[21] and r[23] == "0" for r in one)   # centre to centre: diameter 0
    detect = cells(os.path.join(root, "with", "lesion_detect.csv"))
    assert detect[0] == list(LM.DETECT_COLUMNS) == ["class", "labels", "bin", "labelled", "detected", "invented"]
    assert detect[1:] == R.expected_detect(LITS, want, diams)
    assert [r[2] for r in detect[1:5]] == ["<5", "5-10", "10-20", ">=20"]
    tumour = [r for r in detect[1:] if r[0] == "1"]
    assert sum(int(r[3]) for r in tumour) == 6 and sum(int(r[4]) for r in tumour) == 4   # one missed per subject
    assert sum(int(r[5]) for r in tumour) == 2                                          # and one invented
    for c in (0, 1):
        assert f"[score] class {c} (labels {'1 2' if c == 0 else '2'}), detected / labelled +invented by diameter: <5 mm" in said


def test_score_refuses_an_oblique_map_before_the_device_or_out_dir_is_touched(tmp_path):
    root = str(tmp_path)
    write_score_cases(root, {"tilted": two_maps(3, (7, 9, 8)) + (oblique(),)})

    def never(*a, **k):
        raise AssertionError("a device call ran")
    calls = calls_with_measures(LITS, [])
    calls.tallies = calls.measures = never
    with pytest.raises(SystemExit) as e:
        score.run(score_args(root, "out", "--lesion_measures"), calls=calls)
    assert all(n in str(e.value) for n in ("subject tilted", "--measure_plane d|h|w"))
    assert not os.path.exists(os.path.join(root, "out"))
    seen = []
    score.run(score_args(root, "out", "--lesion_measures", "--measure_plane", "h"), calls=calls_with_measures(LITS, seen))
    assert [s[1] for s in seen] == [1] and {r[22] for r in cells(os.path.join(root, "out", "lesions.csv"))[1:]} == {"h"}


# ---- the predict mission ------------------------------------------------------------------------------------------------------
def test_predict_measures_the_map_it_writes_and_leaves_the_other_files_byte_for_byte(tmp_path, capsys):
    root = str(tmp_path)
    aff = np.array([[0.0, -1.0, 0, 30.0], [1.0, 0.0, 0, -4.0], [0, 0, 2.0, 5.0], [0, 0, 0, 1.0]])
    lst, _ = write_cases(root, ["s2", "s1"], [3, 4], affine=aff, shape=(12, 14, 16), margin=((2, 1), (1, 2), (2, 2)))
    kw = dict(src_list=lst, patch_size="8,8,8", prep_mask="nonzero", post=["1,2:min3"])
    classes = ((1,), (1, 2))
    seen = []

    def measures(labels, truth, lut, C, spacing, slice_axis):
        assert truth is None and labels.dtype == torch.uint8 and list(lut) == Cf.score_class_lut(classes) and C == 2
        nrows, rows, meas, _ = R.measures(labels.numpy(), None, classes, 26, spacing, slice_axis)
        seen.append((labels.numpy().copy(), tuple(spacing), slice_axis))
        return None, torch.from_numpy(nrows), [torch.from_numpy(r) for r in rows], [torch.from_numpy(m) for m in meas]
    predict.run(predict_args(out_dir=os.path.join(root, "plain"), **kw), ops=PostOps(), model=PointNet(), window_batch=3)
    plain = capsys.readouterr().out
    predict.run(predict_args("--lesion_measures", "--measure_class", "1", "--measure_class", "1,2",
                             out_dir=os.path.join(root, "with"), **kw),
                ops=PostOps(), model=PointNet(), window_batch=3, measures=measures)
    said = capsys.readouterr().out
    assert written(os.path.join(root, "with")) == ["lesions.csv", "predict.csv", "s1.nii.gz", "s2.nii.gz"]
    for name in written(os.path.join(root, "plain")):
        assert read(os.path.join(root, "plain", name)) == read(os.path.join(root, "with", name)), name
    want = []
    for (labels, spacing, axis), sn in zip(seen, ("s1", "s2")):
        assert np.array_equal(labels, nifti.read_nifti(os.path.join(root, "with", f"{sn}.nii.gz"))[0])   # after --post
        assert spacing == (1.0, 1.0, 2.0) and axis == 2
        _, rows, meas, _ = R.measures(labels, None, classes, 26, spacing, axis)
        full, _ = R.expected_lesions(sn, classes, False, rows, meas, labels.shape, spacing, aff, axis)
        want += [r[:9] + r[10:] for r in full]
    got = cells(os.path.join(root, "with", "lesions.csv"))
    assert got[0] == [k for k in R.COLUMNS if k != "overlap"]
    assert got[1:] == want and want and {r[3] for r in want} == {"pred"}
    # the per-subject line gains the lesion counts; every other line is what it was
    lines, before = said.splitlines(), plain.replace(os.path.join(root, "plain"), os.path.join(root, "with")).splitlines()
    for sn in ("s1", "s2"):
        n = [sum(1 for r in want if r[0] == sn and r[1] == str(c)) for c in (0, 1)]
        mine = [ln for ln in lines if ln.startswith(f"[predict] {sn}:")]
        assert len(mine) == 1 and f", lesions class 0 (1): {n[0]}, class 1 (1 2): {n[1]}" in mine[0]
        assert mine[0].replace(f", lesions class 0 (1): {n[0]}, class 1 (1 2): {n[1]}", "") in before
    assert [ln for ln in lines if "lesions" not in ln] == [ln for ln in before if not ln.startswith(("[predict] s1:",
                                                                                                     "[predict] s2:"))]


def test_predict_refuses_the_limits_and_an_oblique_scan_before_the_device_is_touched(tmp_path, monkeypatch):
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst, _ = write_cases(root, ["big"], [5], affine=oblique(), shape=(12, 14, 16), margin=((2, 1), (1, 2), (2, 2)))
    kw = dict(src_list=lst, out_dir=out, patch_size="8,8,8", prep_mask="nonzero")

    def never(*a, **k):
        raise AssertionError("the device call ran")
    with pytest.raises(SystemExit) as e:
        predict.run(predict_args("--lesion_measures", **kw), ops=PredictOps(), model=PointNet(), measures=never)
    assert all(n in str(e.value) for n in ("subject big", "--measure_plane d|h|w")) and not os.path.exists(out)
    monkeypatch.setattr(_lib, "EDT_MM_MAX_EXTENT", 15)
    with pytest.raises(SystemExit) as e:
        predict.run(predict_args("--lesion_measures", "--measure_plane", "d", **kw), ops=PredictOps(), model=PointNet(),
                    measures=never)
    assert all(n in str(e.value) for n in ("subject big", "--lesion_measures", "12 14 16", "15")) and not os.path.exists(out)
    # the other limit: the class planes of the subject hold 2^31 voxels or more (the header alone says so)
    monkeypatch.undo()
    plan_of = prep.PrepOptions.plan

    def huge(self, entry, mods):
        plan = plan_of(self, entry, mods)
        plan.source_shape = (1024, 1024, 1024)
        return plan
    monkeypatch.setattr(prep.PrepOptions, "plan", huge)
    with pytest.raises(SystemExit) as e:
        predict.run(predict_args("--lesion_measures", "--measure_plane", "d", **kw), ops=PredictOps(), model=PointNet(),
                    measures=never)
    assert all(n in str(e.value) for n in ("subject big", "--lesion_measures", "2 masks", "1024 1024 1024", "2^31"))
    assert not os.path.exists(out)


def test_a_class_without_lesions_gives_no_rows():
    empty = [np.zeros((0, 3), np.int32)], [np.zeros((0, R.WORDS), np.int64)]
    assert LM.lesion_rows("s", ((3,),), False, *empty, (4, 4, 4), (1.0, 1.0, 1.0), np.eye(4), 2) == []
    assert R.expected_lesions("s", ((3,),), False, *empty, (4, 4, 4), (1.0, 1.0, 1.0), np.eye(4), 2) == ([], [])
    assert [r["labelled"] for r in LM.detect_rows(((3,),), [])] == [0, 0, 0, 0]


def test_a_map_beyond_the_bound_of_the_search_stops_the_mission_naming_the_subject(tmp_path):
    root = str(tmp_path)
    write_score_cases(root, {"noisy": two_maps(3, (7, 9, 8)) + (PLAIN,)})
    calls = calls_with_measures(LITS, [])

    def beyond(*a, **k):
        raise _lib.EffqError("label_lesion_measures: more pairs of tiles than one launch takes: not searched")
    calls.measures = beyond
    with pytest.raises(SystemExit) as e:
        score.run(score_args(root, "out", "--lesion_measures"), calls=calls)
    assert all(n in str(e.value) for n in ("subject noisy", "--lesion_measures", "not searched"))
    assert _lib.LESION_MEASURE_MAX_TILE_PAIRS == 1 << 26
    with open(os.path.join(ROOT, "include", "effq_hip.h")) as f:
        assert "#define EFFQ_LESION_MEASURE_MAX_TILE_PAIRS (1ll << 26)" in f.read()
