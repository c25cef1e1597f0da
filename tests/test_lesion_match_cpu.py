"""One-to-one lesion matching without a GPU (-m "not gpu"): efficientq_amd.lesion_match against the dense restatement of
tests/lesion_match_ref.py on seeded random masks and on hand-made cases, the CSV writers, the refusals of --lesion_match,
the flag and the YAML key, the header against _lib.SIGNATURES, the Makefile, and the surface of HipOps."""
import csv
import inspect
import os
import re

import numpy as np
import pytest

from efficientq_amd import _lib, config as Cf, entrance, evaluate as E, lesion_match as LM, ops_match
from efficientq_amd.hip_ops import HipOps
from tests.lesion_match_ref import ref_pairs, ref_scores
from tests.test_lesion_table_cpu import _ctype, _results
from tests.test_ops_layout_cpu import SURFACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _compare(a, b, pairs):
    got, want = LM.match_class(a, b, pairs), ref_scores(a, b, pairs)
    for k in ("tp_l", "fp_l", "fn_l", "groups"):
        assert got[k] == want[k], k
    for k in LM.SCORES:
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    pr = np.asarray(pairs, np.int64).reshape(-1, 3)
    assert [(int(i), int(j)) for i, j in pr[got["matched"], :2]] == want["matches"]
    for side in ("label", "pred"):
        assert got[side]["match"].tolist() == want[side]["match"], side
        assert got[side]["partners"].tolist() == want[side]["partners"], side
        assert np.abs(got[side]["best_iou"] - np.array(want[side]["best_iou"], np.float64)).max(initial=0.0) <= TOL
    # the groups, lesion by lesion: group g of the code holds the lesions of the g-th group of the flood fill
    for g, (gl, gp) in enumerate(want["group_sets"]):
        assert np.flatnonzero(got["label"]["group"] == g + 1).tolist() == gl
        assert np.flatnonzero(got["pred"]["group"] == g + 1).tolist() == gp
    assert int((got["label"]["group"] == 0).sum()) == want["label"]["partners"].count(0)
    assert int((got["pred"]["group"] == 0).sum()) == want["pred"]["partners"].count(0)
    # uniqueness: no lesion in two matches
    m = pr[got["matched"]]
    assert len(set(m[:, 0].tolist())) == len(m) == len(set(m[:, 1].tolist()))
    return got, want


# ---- against the dense restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dl,dp", [(0.02, 0.02), (0.06, 0.1), (0.15, 0.12), (0.3, 0.3), (0.08, 0.5)])
def test_random_masks_against_the_dense_restatement(dl, dp):
    shape = (12, 14, 16)
    rng = np.random.default_rng(int(1000 * dl + 7 * 1000 * dp))
    gt = rng.random(shape) < dl
    pred = (rng.random(shape) < dp) | (gt & (rng.random(shape) < 0.7))      # correlated, so that some lesions match
    a, b, pairs = ref_pairs(pred, gt)
    assert pairs[:, 2].sum() == (gt & pred).sum() and len(a) > 0 and len(b) > 0
    got, _ = _compare(a, b, pairs)
    shuffled = pairs[rng.permutation(len(pairs))]                          # the scores do not depend on the order
    again = LM.match_class(a, b, shuffled)
    for k in ("tp_l", "fp_l", "fn_l", "groups"):
        assert again[k] == got[k]
    for k in LM.SCORES:
        assert abs(again[k] - got[k]) <= TOL


def test_sparse_blobs_match_and_score_between_zero_and_one():
    """Boxes shifted by one voxel: every label box has exactly one partner, most of them matched."""
    gt = np.zeros((12, 14, 16), bool)
    pred = np.zeros_like(gt)
    for k, (d, h, w) in enumerate([(1, 1, 1), (1, 8, 8), (7, 2, 9), (7, 9, 2)]):
        gt[d:d + 3, h:h + 3, w:w + 4] = True
        pred[d:d + 3, h:h + 3, w + (k % 3):w + 4 + (k % 3)] = True
    a, b, pairs = ref_pairs(pred, gt)
    got, _ = _compare(a, b, pairs)
    assert len(pairs) == 4 and got["groups"] == 4
    # shifts 0, 1, 2, 0 of a width of 4: IoU 1, 3/5, 1/3, 1
    assert got["iou"].tolist() == [1.0, 27 / 45, 18 / 54, 1.0] and got["tp_l"] == 3 and got["fp_l"] == got["fn_l"] == 1
    assert abs(got["sq"] - (1 + 0.6 + 1) / 3) <= TOL and abs(got["pq"] - 2.6 / 4) <= TOL
    assert abs(got["lw_dsc"] - (1 + 2 * 27 / 72 + 2 * 18 / 72 + 1) / 4) <= TOL


# ---- hand cases -----------------------------------------------------------------------------------------------------
def _empty_pairs():
    return np.zeros((0, 3), np.int64)


def test_both_masks_empty():
    got, _ = _compare([], [], _empty_pairs())
    assert (got["tp_l"], got["fp_l"], got["fn_l"], got["groups"]) == (0, 0, 0, 0)
    assert [got[k] for k in LM.SCORES] == [1.0, 1.0, 1.0, 1.0]


def test_label_only_and_prediction_only():
    got, _ = _compare([5, 9], [], _empty_pairs())
    assert (got["tp_l"], got["fp_l"], got["fn_l"]) == (0, 0, 2) and [got[k] for k in LM.SCORES] == [0.0] * 4
    assert got["label"]["match"].tolist() == [0, 0] and got["label"]["partners"].tolist() == [0, 0]
    got, _ = _compare([], [4], _empty_pairs())
    assert (got["tp_l"], got["fp_l"], got["fn_l"]) == (0, 1, 0) and [got[k] for k in LM.SCORES] == [0.0] * 4


def test_one_prediction_over_three_label_lesions():
    a, b = [10, 10, 10], [40]
    pairs = [[0, 0, 10], [1, 0, 10], [2, 0, 10]]
    got, _ = _compare(a, b, pairs)
    assert (got["tp_l"], got["fp_l"], got["fn_l"], got["groups"]) == (0, 1, 3, 1)      # IoU 1/4 each: nothing matches
    assert got["pred"]["partners"].tolist() == [3] and got["label"]["partners"].tolist() == [1, 1, 1]
    assert got["f1_l"] == got["sq"] == got["pq"] == 0.0 and abs(got["lw_dsc"] - 60 / 70) <= TOL
    assert got["pred"]["best_iou"].tolist() == [0.25]


def test_three_predictions_in_one_label_lesion():
    a, b = [30], [5, 20, 5]
    pairs = [[0, 0, 5], [0, 1, 20], [0, 2, 5]]
    got, _ = _compare(a, b, pairs)
    assert (got["tp_l"], got["fp_l"], got["fn_l"], got["groups"]) == (1, 2, 0, 1)      # 20 / 30 > 1/2: the middle one
    assert got["label"]["match"].tolist() == [2] and got["pred"]["match"].tolist() == [0, 1, 0]
    assert abs(got["sq"] - 2 / 3) <= TOL and abs(got["pq"] - (2 / 3) / 2) <= TOL and got["lw_dsc"] == 1.0
    assert abs(got["f1_l"] - 0.5) <= TOL


def test_the_tie_at_one_half_is_left_unmatched_on_both_sides():
    """A label lesion of two voxels, each of them a predicted lesion of its own: IoU 1/2 with both.  With >= the label
    lesion would be in two matches; strict > matches none."""
    got, _ = _compare([2], [1, 1], [[0, 0, 1], [0, 1, 1]])
    assert got["iou"].tolist() == [0.5, 0.5] and not got["matched"].any()
    assert (got["tp_l"], got["fp_l"], got["fn_l"]) == (0, 2, 1)
    assert got["label"]["match"].tolist() == [0] and got["pred"]["match"].tolist() == [0, 0]
    assert got["label"]["best_iou"].tolist() == [0.5] and got["lw_dsc"] == 1.0
    # the same from masks: the two voxels are not adjacent in the prediction's own mask only if something separates
    # them, so the label is a bar of three whose middle voxel is not predicted
    gt = np.zeros((1, 1, 5), bool)
    gt[0, 0, 1:4] = True
    pred = np.zeros_like(gt)
    pred[0, 0, [0, 1, 3, 4]] = True                    # two lesions of two voxels, one voxel of each in the label
    a, b, pairs = ref_pairs(pred, gt)
    assert a.tolist() == [3] and b.tolist() == [2, 2] and pairs.tolist() == [[0, 0, 1], [0, 1, 1]]
    got, _ = _compare(a, b, pairs)
    assert got["iou"].tolist() == [0.25, 0.25]


def test_a_chain_is_one_group():
    """L1 - P1 - L2 - P2: three pairs, one group."""
    a, b = [6, 8], [7, 5]
    pairs = [[0, 0, 3], [1, 0, 2], [1, 1, 4]]
    got, _ = _compare(a, b, pairs)
    assert got["groups"] == 1 and abs(got["lw_dsc"] - 2 * 9 / 26) <= TOL
    assert got["label"]["group"].tolist() == [1, 1] and got["pred"]["group"].tolist() == [1, 1]
    assert got["tp_l"] == 0 and got["label"]["partners"].tolist() == [1, 2] and got["pred"]["partners"].tolist() == [2, 1]
    # with a loose lesion on each side the mean is over three
    got, _ = _compare(a + [4], b + [9], pairs)
    assert got["groups"] == 1 and abs(got["lw_dsc"] - (2 * 9 / 26) / 3) <= TOL


def test_bad_pairs_are_refused():
    with pytest.raises(ValueError):
        LM.match_class([3], [3], [[0, 1, 1]])
    with pytest.raises(ValueError):
        LM.match_class([3], [3], [[0, 0, 0]])


# ---- the CSV writers ------------------------------------------------------------------------------------------------
def _matched_results():
    """The results of test_lesion_table_cpu with a matching that fits their sizes: s1 class 0 has one pair."""
    res = _results()
    for r in res:
        r["lesion_match"] = []
        for lab_rows, pred_rows in r["lesion_table"]:
            a, b = lab_rows[:, 3], pred_rows[:, 3]
            pairs = [[1, 0, 7]] if len(a) == 2 and len(b) == 1 else []
            m = LM.match_class(a, b, pairs)
            m["pairs"] = np.array(pairs, np.int64).reshape(-1, 3)
            r["lesion_match"].append(m)
    return res


def test_lesions_csv_is_unchanged_without_the_key_and_gains_three_columns_with_it(tmp_path):
    path = str(tmp_path / "lesions.csv")
    E.write_lesions_csv(path, _results())
    want = "subject,class,kind,lesion,d,h,w,size,overlap\r\n" + "".join(
        f"{r['name']},{c},{kind},{k + 1},{','.join(str(int(v)) for v in row)}\r\n"
        for r in _results() for c, pair in enumerate(r["lesion_table"]) for kind, rows in zip(("label", "pred"), pair)
        for k, row in enumerate(rows))
    assert open(path, "rb").read() == want.encode()
    E.write_lesions_csv(path, _results((2.0, 1.0, 0.5)))
    assert list(csv.reader(open(path)))[0][-1] == "vol_mm3"

    res = _matched_results()
    E.write_lesions_csv(path, res)
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["subject", "class", "kind", "lesion", "d", "h", "w", "size", "overlap", "match", "best_iou",
                       "partners"]
    iou = "%.7g" % (7 / (120 + 30 - 7))
    assert rows[1] == ["s1", "0", "label", "1", "0", "1", "2", "5", "0", "0", "0", "0"]
    assert rows[2] == ["s1", "0", "label", "2", "3", "0", "0", "120", "7", "0", iou, "1"]
    assert rows[3] == ["s1", "0", "pred", "1", "3", "0", "1", "30", "7", "0", iou, "1"]
    for r in res:
        r["spacing"] = (2.0, 1.0, 0.5)
    E.write_lesions_csv(path, res)
    assert list(csv.reader(open(path)))[0][-4:] == ["vol_mm3", "match", "best_iou", "partners"]
    del res[0]["lesion_match"]
    with pytest.raises(RuntimeError):
        E.write_lesions_csv(path, res)


def test_match_and_pairs_csv_columns(tmp_path):
    res = _matched_results()
    res[1]["lesion_match"][0] = dict(LM.match_class([9, 10], [9], [[0, 0, 9]]), pairs=np.array([[0, 0, 9]], np.int64))
    a, b = str(tmp_path / "lesion_match.csv"), str(tmp_path / "lesion_pairs.csv")
    LM.write_lesion_match_csv(a, res)
    LM.write_lesion_pairs_csv(b, res)
    rows = list(csv.reader(open(a)))
    assert rows[0] == ["subject", "class", "tp_l", "fp_l", "fn_l", "f1_l", "sq", "pq", "lw_dsc", "groups"]
    assert len(rows) == 1 + 4
    assert rows[1] == ["s1", "0", "0", "1", "2", "0", "0", "0", "%.7g" % ((14 / 150) / 2), "1"]
    assert rows[2] == ["s1", "1", "0", "1", "0", "0", "0", "0", "0", "0"]
    assert rows[3] == ["s2", "0", "1", "0", "1", "%.7g" % (2 / 3), "1", "%.7g" % (1 / 1.5), "0.5", "1"]
    prs = list(csv.reader(open(b)))
    assert prs[0] == ["subject", "class", "label_lesion", "pred_lesion", "overlap", "iou"]
    assert prs[1:] == [["s1", "0", "2", "1", "7", "%.7g" % (7 / 143)], ["s2", "0", "1", "1", "9", "1"]]
    s = LM.match_summary(res)
    assert [m["tp_l"] for m in s] == [1, 0] and [m["fp_l"] for m in s] == [1, 1] and [m["fn_l"] for m in s] == [3, 1]
    assert abs(s[0]["f1_l"] - (0 + 2 / 3) / 2) <= TOL


# ---- the switch -----------------------------------------------------------------------------------------------------
def test_parser_knows_lesion_match_and_a_yaml_key_sets_it(tmp_path):
    assert Cf.build_parser().parse_args(["ptq"]).lesion_match is False
    assert Cf.build_parser().parse_args(["ptq", "--lesion_match"]).lesion_match is True
    assert Cf.make_args(Cf.TINY_NET, 4, 4).lesion_match is False
    cfg = tmp_path / "match.yaml"
    cfg.write_text("lesion_match: true\ntask: lits\n")
    args = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"]))
    assert args.lesion_match is True and args.lesion_table is False
    assert Cf.match_switches(args) is True
    assert Cf.match_switches(Cf.build_parser().parse_args(["ptq"])) is False


@pytest.mark.parametrize("argv,text", [
    (["ptq", "--lesion_match", "--unlabelled", "--vs_fp"], "--lesion_match --unlabelled: predicted lesions are matched"),
    (["ptq", "--lesion_match", "--synthetic"], "--lesion_match --synthetic: predicted lesions are matched to labelled"),
    (["ptq", "--lesion_match", "--no_test"], "--lesion_match --no_test: the matching belongs to the validation"),
    (["prep", "--lesion_match"], "the prep mission validates nothing, drop --lesion_match"),
    (["predict", "--lesion_match"], "the predict mission validates nothing, drop --lesion_match"),
])
def test_refusals_name_the_switches_before_anything_runs(argv, text, tmp_path):
    with pytest.raises(SystemExit) as e:
        entrance.main(argv)
    assert text in str(e.value)
    cfg = tmp_path / "match.yaml"                      # the YAML key is refused alike
    cfg.write_text("lesion_match: true\n")
    with pytest.raises(SystemExit) as e:
        entrance.main([a for a in argv if a != "--lesion_match"] + ["--config", str(cfg)])
    assert text in str(e.value)


def test_do_ptq_passes_is_match_only_when_set():
    src = inspect.getsource(__import__("efficientq_amd.calibrate", fromlist=["do_ptq"]).do_ptq)
    assert re.search(r"if getattr\(args, 'lesion_match', False\):\s+cc\['is_match'\] = True", src)
    sig = inspect.signature(entrance._ValidationTester.test_as_is)
    assert sig.parameters["is_match"].default is False
    assert inspect.signature(E.validate_seg).parameters["lesion_match"].default is False


# ---- the symbols, the build and the surface ---------------------------------------------------------------------------
def test_match_symbols_in_header_and_lib_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, res in (("effq_seg_lesion_match_ws_bytes", "size_t"), ("effq_seg_lesion_match", "int")):
        m = re.search(rf"\b{res} {name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        got_res, got = _lib.SIGNATURES[name]
        assert got == [_ctype(a) for a in m.group(1).split(",")], name
        assert got_res == (_lib._SZ if res == "size_t" else _lib._I)
    assert len(_lib.SIGNATURES["effq_seg_lesion_match"][1]) == 20
    # the arguments of the table, then max_pairs, the table's outputs, the pairs', and the workspace
    table, match = _lib.SIGNATURES["effq_seg_lesion_table"][1], _lib.SIGNATURES["effq_seg_lesion_match"][1]
    assert match[:11] == table[:11] and match[11] == _lib._I and match[12:15] == table[11:14]
    assert match[15:17] == [_lib._P, _lib._P] and match[17:] == table[14:]
    assert _lib.LESION_PAIR_ROWS > 0


def test_the_makefile_lists_the_new_source_and_the_header_is_shared():
    csrc = os.path.join(ROOT, "efficientq_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert srcs.count("seg_cc_match.hip") == 1
    src = open(os.path.join(csrc, "seg_cc_match.hip")).read()
    assert '#include "seg_cc.h"' in src
    for fn in ("effq_seg_lesion_match_ws_bytes", "effq_seg_lesion_match"):
        assert len(re.findall(rf"^(?:int|size_t) {fn}\s*\([^;{{]*\)\s*\{{", src, re.M)) == 1, fn
    hdr = open(os.path.join(csrc, "seg_cc.h")).read()
    assert re.search(r"^int cc_table_run\s*\(", hdr, re.M) and "struct CcTableWs" in hdr
    table = open(os.path.join(csrc, "seg_cc_table.hip")).read()
    assert "struct CcTableWs" not in table and "static int cc_table_run" not in table
    # the row of a voxel is written once and used by the table and by the pairs
    assert len(re.findall(r"-L\[l - 1\] - 1", hdr + table + src)) == 1 and "cc_row(" in table and "cc_row(" in src


def test_ops_match_is_a_function_and_hip_ops_has_no_new_attribute():
    assert inspect.isfunction(ops_match.seg_lesion_match)
    params = list(inspect.signature(ops_match.seg_lesion_match).parameters)
    assert params == ["ops", "logits", "label", "task", "fuse", "max_rows", "max_pairs"]
    assert not any("match" in name for name in dir(HipOps))
    assert [n for n in dir(HipOps) if not n.startswith("__")] == [name for name, _ in SURFACE]
