"""--thr_sweep and --thresh, host side (no GPU): the edges of effq_seg_sweep_edges against the restatement's, the integer
AUC of sweep_summary against scikit-learn, its suffix sums and tie rule, the switches and what they refuse, the argument
checks of the C ABI (which run before anything is launched), and the validation, the ptq tester and the predict mission
driven through stand-ins for the device ops."""
import csv
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, entrance, evaluate as E, nifti, predict
from tests import seg_sweep_ref as R
from tests.test_post_cpu import BratsNet, PostOps, SpeckNet, _lits_loader
from tests.test_predict_cpu import PointNet, predict_args, ref_merge, write_cases
from tests.test_prep_cpu import written

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESH = float(np.float32(-1.7881393e-07))      # what sigmoid_threshold() finds on the device: not 0, a little below it
ARG = 1


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def _lib_edges(mode, thresh):
    out = (C.c_float * 4096)()
    assert _lib.load().effq_seg_sweep_edges(mode, thresh, out) == 0
    return np.frombuffer(bytearray(out), dtype=np.float32)


def test_edges_of_the_library_are_the_restatements_bit_for_bit():
    for mode, name, t in ((_lib.SEG_SIGMOID, "sigmoid", THRESH), (_lib.SEG_ARGMAX, "argmax", 0.0),
                          (_lib.SEG_SIGMOID, "sigmoid", 0.005), (_lib.SEG_ARGMAX, "argmax", 123.0)):
        got, want = _lib_edges(mode, t), R.edges(name, t)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, t)
        assert got[0] == -np.inf and got[1] == -2047 / 128 and got[4095] == 2047 / 128
        assert (np.diff(got[1:]) > 0).all()
    assert _lib_edges(_lib.SEG_SIGMOID, THRESH)[2048] == np.float32(THRESH) != 0.0
    assert _lib_edges(_lib.SEG_ARGMAX, THRESH)[2048] == 0.0
    assert _lib.SEG_SWEEP_BINS == E.SWEEP_BINS == R.BINS == 4096 and E.SWEEP_MID == R.MID == 2048


def test_new_symbols_in_header_makefile_and_lib():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define EFFQ_SEG_SWEEP_BINS 4096\b", code)
    lib = _lib.load()

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _lib._IP if decl.startswith("int*") else _lib._P
        if decl.startswith("long long"):
            return _lib._LL
        return {"int": _lib._I, "float": _lib._F}[decl.split()[0]]
    for name, nargs in (("effq_seg_sweep", 9), ("effq_seg_sweep_edges", 3), ("effq_seg_sweep_plan", 5)):
        found = re.findall(rf"\bint ({name})\s*\((.*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1, name
        res, got = _lib.SIGNATURES[name]
        assert res == _lib._I and got == [ctype(a) for a in found[0][1].split(",")] and len(got) == nargs
        assert hasattr(lib, name)
    assert "seg_sweep.hip" in open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "efficientq_amd", "csrc", "seg_sweep.hip")).read()
    assert '#include "seg_decide.h"' in src and "predict<MODE, C>" in src
    assert not re.search(r"atomic\w*\s*\(\s*(reinterpret_cast<)?\s*(float|double)", src)      # integer atomics only


def test_argument_checks_run_before_anything_is_launched():
    """No device is needed to be refused: the pointers below are never followed."""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)

    def sweep(Cc=3, S=1000, mode=_lib.SEG_SIGMOID, fuse=0, thresh=THRESH, **null):
        return lib.effq_seg_sweep(null.get("logits", fake), null.get("label", fake), Cc, S, mode, fuse, thresh,
                                  null.get("hist", fake), None)
    for name in ("logits", "label", "hist"):
        assert sweep(**{name: None}) == ARG, name
    assert "argument check failed" in lib.effq_last_error().decode()
    assert sweep(Cc=0) == ARG and sweep(Cc=9) == ARG and sweep(Cc=-1) == ARG
    assert sweep(S=0) == ARG and sweep(S=2 ** 31) == ARG and sweep(S=-5) == ARG
    assert sweep(mode=2) == ARG and sweep(fuse=3) == ARG and sweep(fuse=-1) == ARG
    for fuse in (1, 2):
        assert sweep(mode=_lib.SEG_ARGMAX, fuse=fuse) == ARG                  # a merge needs the sigmoid mode
    e = R.edges("sigmoid", THRESH)
    for t in (float(e[2047]), float(e[2049]), 0.5, -0.5, float("nan"), float("inf"), -float("inf")):
        assert sweep(thresh=t) == ARG, t
    assert sweep(logits=C.c_void_p(0x1002)) == ARG and sweep(hist=C.c_void_p(0x1004)) == ARG      # alignment
    out = (C.c_float * 4096)()
    assert lib.effq_seg_sweep_edges(_lib.SEG_SIGMOID, float(e[2049]), out) == ARG
    assert lib.effq_seg_sweep_edges(_lib.SEG_SIGMOID, float("nan"), out) == ARG
    assert lib.effq_seg_sweep_edges(2, 0.0, out) == ARG and lib.effq_seg_sweep_edges(_lib.SEG_SIGMOID, 0.0, None) == ARG
    assert lib.effq_seg_sweep_edges(_lib.SEG_SIGMOID, float(np.nextafter(e[2049], np.float32(0))), out) == 0
    grid, trips = C.c_int(-1), C.c_int(-1)
    plan = lambda Cc, S, mode=0: lib.effq_seg_sweep_plan(Cc, S, mode, C.byref(grid), C.byref(trips))
    assert plan(0, 100) == ARG and plan(9, 100) == ARG and plan(3, 0) == ARG and plan(3, 2 ** 31) == ARG
    assert plan(3, 100, 7) == ARG and lib.effq_seg_sweep_plan(3, 100, 0, None, C.byref(trips)) == ARG
    assert (grid.value, trips.value) == (-1, -1)
    # the plan: voxel ranges of 512 groups of four voxels, 256 at most, times the class pairs
    for Cc, S, want in ((1, 1, (1, 0)), (3, 3, (2, 0)), (2, 4, (1, 1)), (3, 4099, (4, 1)), (8, 4 * 512 * 256, (1024, 1)),
                        (8, 4 * 512 * 256 + 4, (1024, 2)), (3, 155 * 240 * 240, (512, 18)), (5, 2 ** 31 - 1, (768, 4096))):
        assert plan(Cc, S) == 0 and (grid.value, trips.value) == want, (Cc, S)


# ---- sweep_summary --------------------------------------------------------------------------------------------------------
def _random_case(seed, S=200_003, prevalence=0.1):
    rng = np.random.default_rng(seed)
    truth = rng.random(S) < prevalence
    score = (rng.standard_normal(S) + 1.8 * truth).astype(np.float32)
    score[rng.random(S) < 0.01] = np.float32(np.nan)
    score[rng.random(S) < 0.3] = np.float32(-30.0)            # background far below the first edge
    return truth, score


def _hist_of(truth, score, e):
    b = R.bins_of(score, e)
    hist = np.zeros((1, 2, 4096), dtype=np.int64)
    np.add.at(hist[0], (truth.astype(np.int64), b), 1)
    return hist, b


def test_auc_is_scikit_learns_on_the_bins():
    metrics = pytest.importorskip("sklearn.metrics")
    e = R.edges("sigmoid", THRESH)
    for seed, prevalence in ((1, 0.1), (2, 0.5), (3, 0.001)):
        truth, score = _random_case(seed, prevalence=prevalence)
        hist, b = _hist_of(truth, score, e)
        got = E.sweep_summary(hist, e)[0]["auc"]
        assert abs(got - metrics.roc_auc_score(truth, b)) <= 1e-12
        assert 0.5 < got < 1.0
    # all positives in one bin, negatives on both sides of it and inside it
    truth = np.array([1] * 50 + [0] * 150, dtype=bool)
    score = np.concatenate([np.full(50, 0.3), np.full(40, 0.3), np.full(60, -2.0), np.full(50, 4.0)]).astype(np.float32)
    hist, b = _hist_of(truth, score, e)
    got = E.sweep_summary(hist, e)[0]["auc"]
    assert abs(got - metrics.roc_auc_score(truth, b)) <= 1e-12 and got == (2 * 50 * 60 + 50 * 40) / (2 * 50 * 150)


def test_auc_by_hand_and_with_one_class_of_truth_absent():
    e = R.edges("argmax")
    hist = np.zeros((3, 2, 4096), dtype=np.int64)
    hist[0, 1, 2050] = 7                                        # positives only
    hist[1, 0, 10] = 9                                          # negatives only
    hist[2, 0, 100], hist[2, 0, 200], hist[2, 1, 200], hist[2, 1, 300] = 3, 1, 2, 4
    s = E.sweep_summary(hist, e)
    assert s[0]["auc"] == 1.0 and s[1]["auc"] == 1.0 and (s[0]["pos"], s[0]["neg"], s[1]["pos"], s[1]["neg"]) == (7, 0, 0, 9)
    # class 2: pairs (pos, neg): 2 x 3 above + 2 x 1 tied + 4 x 4 above = 22 + 1 of 24
    assert s[2]["auc"] == (2 * (2 * 3 + 4 * 4) + 2 * 1) / (2 * 6 * 4) == 46 / 48
    # pooled counts beyond 2^63 in the numerator: Python integers carry them
    big = [[[0] * 4096, [0] * 4096]]
    big[0][0][5], big[0][1][9] = 2 ** 40, 2 ** 40
    assert E.sweep_summary(big, e)[0]["auc"] == 1.0
    big[0][0][9] = 2 ** 40
    assert E.sweep_summary(big, e)[0]["auc"] == 0.75
    pooled = E.sweep_pooled([hist, hist, torch.from_numpy(hist)])
    assert pooled[2][1][300] == 12 and E.sweep_summary(pooled, e)[2]["auc"] == 46 / 48


def test_suffix_sums_are_direct_counts_of_the_decision():
    e = R.edges("sigmoid", THRESH)
    truth, score = _random_case(5)
    hist, _ = _hist_of(truth, score, e)
    s = E.sweep_summary(hist, e)[0]
    assert s["counts"].dtype == torch.int64 and tuple(s["counts"].shape) == (4096, 4)
    assert s["counts"][0].tolist() == [int(truth.sum()), int((~truth).sum()), 0, 0]
    for k in (1, 2, 1024, 2047, 2048, 2049, 2100, 2300, 4095):
        with np.errstate(invalid="ignore"):
            pred = score >= e[k]                                # NaN is below every edge
        want = [int((pred & truth).sum()), int((pred & ~truth).sum()), int((~pred & truth).sum()), int((~pred & ~truth).sum())]
        assert s["counts"][k].tolist() == want, k
        assert np.array_equal(R.decision_counts(hist, k)[0], want)
    m = E.metrics_from_counts(s["counts"][[2048, s["best_k"]]])
    assert float(s["dsc_default"]) == float(m["dsc"][0]) and float(s["dsc_best"]) == float(m["dsc"][1])
    assert float(s["sens_best"]) == float(m["sens"][1]) and float(s["spec_best"]) == float(m["spec"][1])
    assert s["best_thr"] == float(e[s["best_k"]]) and float(s["dsc_best"]) > float(s["dsc_default"])
    # the best k is the argmax of the fp64 Dice over all rows
    c = s["counts"].numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = 2 * c[1:, 0] / (2 * c[1:, 0] + c[1:, 1] + c[1:, 2])
    assert d[s["best_k"] - 1] == np.nanmax(d)


def test_tie_rule_of_the_best_threshold():
    e = R.edges("sigmoid", THRESH)

    def best(pos=(), neg=()):
        hist = np.zeros((1, 2, 4096), dtype=np.int64)
        for b, n in pos:
            hist[0, 1, b] += n
        for b, n in neg:
            hist[0, 0, b] += n
        return E.sweep_summary(hist, e)[0]["best_k"]
    # positives in bin 2100, negatives in bin 1900: every k in 1901 .. 2100 separates them; the nearest to 2048 wins
    assert best(pos=[(2100, 5)], neg=[(1900, 5)]) == 2048
    # the plateau lies above 2048: its lower end is the nearest
    assert best(pos=[(3000, 5)], neg=[(2500, 5)]) == 2501
    # below: its upper end
    assert best(pos=[(1500, 5)], neg=[(1000, 5)]) == 1500
    # two rows of equal Dice at equal distance from 2048, lower rows between them: the lower k.  Positives in the bins
    # 2038 and 2058, two negatives in bin 2057: k <= 2038 has TP 2 FP 2 (4 / 6), k in 2039 .. 2057 TP 1 FP 2 FN 1 (2 / 5),
    # k = 2058 TP 1 FN 1 (2 / 3), above nothing is found (0)
    assert best(pos=[(2038, 1), (2058, 1)], neg=[(2057, 2)]) == 2038
    # the same with the upper row one step nearer: it wins
    assert best(pos=[(2038, 1), (2057, 1)], neg=[(2056, 2)]) == 2057
    # a zero denominator counts as -1: with negatives only, the rows k <= 100 have Dice 0 and every other row nothing
    assert best(neg=[(100, 3)]) == 100
    assert best() == 2048                                                     # every row -1
    assert best(pos=[(4095, 2)]) == 2048                                      # every row 1


# ---- the switches ---------------------------------------------------------------------------------------------------------
def _parse(*argv, mission="ptq"):
    return Cf.build_parser().parse_args([mission] + list(argv))


def test_parser_and_yaml_forms(tmp_path):
    a = _parse()
    assert a.thr_sweep is False and a.thresh is None and Cf.thr_switches(a) == (False, None)
    assert Cf.thr_switches(Cf.make_args(Cf.TINY_NET, 4, 4)) == (False, None)          # arguments from before the switches
    a = _parse("--thr_sweep", "--multi_label", "brats", "--thresh", "0.31")
    sweep, t = Cf.thr_switches(a)
    assert sweep is True and t == float(np.float32(math.log(0.31 / 0.69))) and t < 0
    assert Cf.thr_switches(_parse("--multi_label", "brats", "--thresh", "logit:-1.25")) == (False, -1.25)
    assert Cf.thr_switches(_parse("--multi_label", "brats", "--thresh", "logit:0.1"))[1] == float(np.float32(0.1))
    assert Cf.thr_switches(_parse("--multi_label", "brats", "--thresh", "0.9", mission="predict"))[1] > 2.19
    for default in ("0.5", "logit:0", "logit:-0.0", "logit:0.0", "5e-1"):
        assert Cf.thr_switches(_parse("--multi_label", "brats", "--thresh", default)) == (False, None), default
    cfg = tmp_path / "t.yaml"
    cfg.write_text("thr_sweep: true\nthresh: 0.31\nmulti_label: brats\n")
    assert Cf.thr_switches(Cf.merge_config(str(cfg), _parse())) == (True, t)
    cfg.write_text("thresh: 'logit:-1.25'\nmulti_label: brats\n")
    assert Cf.thr_switches(Cf.merge_config(str(cfg), _parse("--thresh", "0.9"))) == (False, -1.25)    # YAML wins
    cfg.write_text("thresh: 0.5\nmulti_label: brats\n")
    assert Cf.thr_switches(Cf.merge_config(str(cfg), _parse())) == (False, None)
    cfg.write_text("thresh: 1.5\nmulti_label: brats\n")
    with pytest.raises(SystemExit) as e:
        Cf.thr_switches(Cf.merge_config(str(cfg), _parse()))
    assert "--thresh" in str(e.value) and "1.5" in str(e.value)


def test_every_edge_reads_back_exactly_from_its_csv_form():
    e = R.edges("sigmoid", THRESH)
    for k in range(1, 4096):
        assert Cf.parse_thresh("logit:%.9g" % e[k]) == float(e[k]), k
    assert Cf.parse_thresh("logit:%.9g" % R.edges("argmax")[2048]) is None
    # a probability is turned into its logit in fp64 and rounded to fp32 once
    assert Cf.parse_thresh("%.17g" % E.logit_prob(2.0)) == 2.0 == float(e[2304])


@pytest.mark.parametrize("argv, named", [
    (["ptq", "--task", "lits", "--thr_sweep", "--unlabelled", "--vs_fp"], ["--thr_sweep", "--unlabelled", "truth"]),
    (["ptq", "--task", "lits", "--thr_sweep", "--synthetic"], ["--thr_sweep", "--synthetic", "truth"]),
    (["ptq", "--task", "lits", "--thr_sweep", "--synthetic", "--vs_fp"], ["--thr_sweep", "--synthetic"]),
    (["ptq", "--task", "lits", "--thr_sweep", "--no_test"], ["--thr_sweep", "--no_test"]),
    (["prep", "--task", "lits", "--thr_sweep"], ["--thr_sweep", "prep"]),
    (["predict", "--task", "lits", "--thr_sweep"], ["--thr_sweep", "predict"]),
    (["prep", "--task", "lits", "--thresh", "0.3", "--multi_label", "brats"], ["--thresh", "prep"]),
    (["ptq", "--task", "lits", "--thresh", "0.3"], ["--thresh", "--multi_label", "argmax"]),
    (["predict", "--task", "lits", "--thresh", "logit:1"], ["--thresh", "--multi_label", "argmax"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "1.5"], ["--thresh", "'1.5'", "between 0 and 1"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "0"], ["--thresh", "'0'", "between 0 and 1"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "1"], ["--thresh", "'1'", "between 0 and 1"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "-0.2"], ["--thresh", "'-0.2'", "between 0 and 1"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "nan"], ["--thresh", "'nan'", "not finite"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "logit:inf"], ["--thresh", "'logit:inf'", "not finite"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "logit:nan"], ["--thresh", "not finite"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "logit:1e39"], ["--thresh", "'logit:1e39'", "fp32"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--thresh", "half"], ["--thresh", "'half'", "logit:X"]),
    (["predict", "--task", "brats", "--multi_label", "brats", "--thresh", "logit:"], ["--thresh", "'logit:'", "logit:X"]),
])
def test_the_missions_refuse_by_name_before_anything_is_created(tmp_path, argv, named):
    snap, data = str(tmp_path / "snap"), str(tmp_path / "data")
    with pytest.raises(SystemExit) as e:
        entrance.main(argv + ["--snap_dir", snap, "--data_dir", data, "--split_dir", str(tmp_path / "split"),
                              "--src_list", str(tmp_path / "none.csv"), "--out_dir", str(tmp_path / "seg"),
                              "--qlvl_w", "4", "--qlvl_a", "4"])
    assert all(n in str(e.value) for n in named), str(e.value)
    assert os.listdir(str(tmp_path)) == []


# ---- stand-ins for the device ---------------------------------------------------------------------------------------------
class SweepOps(PostOps):
    """PostOps with a decision threshold that can be set (default 0.0) and the sweep through the numpy restatement; the
    edges come from the library itself, which needs no device for them."""

    def __init__(self):
        super().__init__()
        self.THRESH = 0.0                       # PredictOps.seg_labels_source decides at it
        self.sweeps = 0

    def default_sigmoid_threshold(self):
        return 0.0

    def sigmoid_threshold(self):
        return self.THRESH

    def set_decision_threshold(self, logit):
        self.THRESH = 0.0 if logit is None else float(np.float32(logit))

    def _bits(self, logits, fuse):
        return ref_merge(logits.numpy() >= np.float32(self.THRESH), fuse)

    def seg_sweep(self, logits, label, task, fuse=None):
        self.sweeps += 1
        x = logits.numpy().reshape(logits.shape[0], -1)
        mode = "argmax" if task == "lits" else "sigmoid"
        return torch.from_numpy(R.sweep(x, label.numpy(), mode, fuse, self.default_sigmoid_threshold()))

    def sweep_edges(self, kind):
        mode = _lib.SEG_ARGMAX if kind in ("lits", "argmax") else _lib.SEG_SIGMOID
        return torch.from_numpy(_lib_edges(mode, self.default_sigmoid_threshold()).copy())


def _brats_loader(n=2, shape=(9, 10, 11)):
    g = torch.Generator().manual_seed(9)
    return [(torch.randn(1, 4, *shape, generator=g), (torch.rand(1, 3, *shape, generator=g) < 0.4).to(torch.uint8))
            for _ in range(n)]


def test_validate_seg_adds_the_histogram_and_leaves_the_rest(monkeypatch):
    from efficientq_amd import hip_ops
    ops = SweepOps()
    monkeypatch.setattr(hip_ops, "get_ops", lambda dev: ops)
    for net, loader, kw in ((SpeckNet(), _lits_loader(), dict(task="lits")),
                            (BratsNet(), _brats_loader(), dict(task="brats", fuse="agg", multi_label="brats"))):
        kw.update(patch_size=(8, 8, 8), overlap=(2, 2, 2), window_batch=4, names=["s1", "s2"])
        base = E.validate_seg(net, loader, **kw)
        assert ops.sweeps == 0
        res = E.validate_seg(net, loader, sweep=True, **kw)
        assert ops.sweeps == 2
        ops.sweeps = 0
        for r0, r, (img, lab) in zip(base, res, loader):
            assert "sweep" not in r0 and sorted(r) == sorted(list(r0) + ["sweep", "sweep_edges"])
            assert all(torch.equal(r0[k], r[k]) for k in ("counts",) + E.METRICS)
            logits, _, _ = E.stitched_window_logits(ops, [net], img, (8, 8, 8), (2, 2, 2), 4)
            x = logits[0][0].numpy()
            mode = "argmax" if kw["task"] == "lits" else "sigmoid"
            want = R.sweep(x.reshape(x.shape[0], -1), lab[0].numpy(), mode, kw.get("fuse"), 0.0)
            assert r["sweep"].dtype == torch.int64 and np.array_equal(r["sweep"].numpy(), want)
            assert np.array_equal(R.decision_counts(want, 2048), r["counts"].numpy())          # row 2048 is metrics.csv
            assert r["sweep_edges"].dtype == torch.float32 and tuple(r["sweep_edges"].shape) == (4096,)
            s = E.sweep_summary(r["sweep"], r["sweep_edges"])
            assert [float(q["dsc_default"]) for q in s] == [float(v) for v in r["dsc"]]


def _cube(loader, multi_label=None, fuse=None):
    return types.SimpleNamespace(valloader=loader, val_sn=["s1", "s2"], patch_size=(8, 8, 8), overlap=(2, 2, 2),
                                 multilabel_fusetype=fuse, multi_label=multi_label, labelled=True, geometry=None,
                                 spacing=None)


@pytest.mark.parametrize("task", ["lits", "brats"])
def test_the_tester_writes_both_files_beside_metrics_csv_and_changes_no_other(tmp_path, monkeypatch, capsys, task):
    from efficientq_amd import hip_ops
    ops = SweepOps()
    monkeypatch.setattr(hip_ops, "get_ops", lambda dev: ops)
    whole = E.validate_seg
    monkeypatch.setattr(E, "validate_seg", lambda *a, **k: whole(*a, window_batch=4, **k))
    if task == "lits":
        net, cube, ncls = SpeckNet(), _cube(_lits_loader()), 3
    else:
        net, cube, ncls = BratsNet(), _cube(_brats_loader(), "brats", "agg"), 3
    rules = [((1,), "min", 3, 0)] if task == "lits" else []
    plain, swept = str(tmp_path / "plain"), str(tmp_path / "swept")
    t0 = entrance._ValidationTester(net, plain, cube, task, post=rules)
    t0.test_as_is("fp")
    t0.test_as_is("ptq")
    assert "thr_sweep" not in capsys.readouterr().out and ops.sweeps == 0
    t1 = entrance._ValidationTester(net, swept, cube, task, post=rules, sweep=True)
    t1.test_as_is("fp")
    said_fp = capsys.readouterr().out
    t1.test_as_is("ptq")
    said = capsys.readouterr().out
    assert "--thr_sweep" in said_fp and "FP: AUC" in said_fp and "PTQ" not in said_fp
    lines = [ln for ln in said.splitlines() if "FP: AUC" in ln and "PTQ: AUC" in ln]
    assert len(lines) == ncls and all("Dice" in ln and " at " in ln for ln in lines)          # both networks side by side
    other = ["metrics.csv"] + (["metrics_post.csv"] if rules else [])
    for folder in ("fp", "ptq"):
        assert written(os.path.join(plain, folder)) == sorted(other)
        assert written(os.path.join(swept, folder)) == sorted(other + ["threshold.csv", "threshold_curve.csv"])
        for f in other:              # every byte of the other files is what it is without the switch
            assert open(os.path.join(plain, folder, f), "rb").read() == open(os.path.join(swept, folder, f), "rb").read()
        with open(os.path.join(swept, folder, "threshold.csv"), newline="") as f:
            thr = list(csv.reader(f))
        with open(os.path.join(swept, folder, "threshold_curve.csv"), newline="") as f:
            curve = list(csv.reader(f))
        with open(os.path.join(swept, folder, "metrics.csv"), newline="") as f:
            met = list(csv.reader(f))
        assert thr[0] == ["subject", "class", "auc", "dsc", "best_thr_logit", "best_thr_prob", "dsc_best", "sens_best",
                          "spec_best", "pos", "neg"]
        assert curve[0] == ["class", "k", "thr_logit", "thr_prob", "tp", "fp", "fn", "tn", "dsc", "sens", "spec"]
        assert [(r[0], r[1]) for r in thr[1:]] == [(s, str(c)) for s in ("s1", "s2", "pooled") for c in range(ncls)]
        assert [(r[0], r[1]) for r in curve[1:]] == [(str(c), str(k)) for c in range(ncls) for k in range(1, 4096)]
        assert [r[3] for r in thr[1:] if r[0] != "pooled"] == [r[2] for r in met[1:]]           # dsc is metrics.csv's
        res = whole(net, cube.valloader, task, (8, 8, 8), (2, 2, 2), names=cube.val_sn, window_batch=4, sweep=True,
                    fuse=cube.multilabel_fusetype, multi_label=cube.multi_label)
        edges = res[0]["sweep_edges"]
        pooled = E.sweep_summary(E.sweep_pooled([r["sweep"] for r in res]), edges)
        nvox = sum(int(np.prod(lab.shape[-3:])) for _, lab in cube.valloader)
        for c, row in enumerate(r for r in thr[1:] if r[0] == "pooled"):
            q = pooled[c]
            assert row[2] == "%.9g" % q["auc"] and row[3] == "%.7g" % float(q["dsc_default"])
            assert np.float32(float(row[4])) == np.float32(q["best_thr"]) == edges[q["best_k"]]
            assert float(row[5]) == pytest.approx(1 / (1 + math.exp(-q["best_thr"])), rel=1e-8)
            assert row[6:9] == ["%.7g" % float(q[k]) for k in ("dsc_best", "sens_best", "spec_best")]
            assert [int(v) for v in row[9:]] == [q["pos"], q["neg"]] and q["pos"] + q["neg"] == nvox
            for k in (1, 2047, 2048, q["best_k"], 4095):
                crow = curve[1 + c * 4095 + k - 1]
                assert [int(v) for v in crow[4:8]] == q["counts"][k].tolist() and sum(int(v) for v in crow[4:8]) == nvox
                assert np.float32(float(crow[2])) == edges[k]
                m = E.metrics_from_counts(q["counts"][k][None])
                assert crow[8:] == ["%.7g" % float(m[j][0]) for j in ("dsc", "sens", "spec")]
            total = np.sum([[int(v) for v in r[6:10]] for r in met[1:] if r[1] == str(c)], axis=0)
            assert curve[1 + c * 4095 + 2047][4:8] == [str(v) for v in total]                  # row 2048: metrics.csv summed


# ---- predict --------------------------------------------------------------------------------------------------------------
def _predict(tmp_path, name, *extra):
    root, out = str(tmp_path), str(tmp_path / name)
    lst = os.path.join(root, "cases.csv")
    if not os.path.exists(lst):
        lst, _ = write_cases(root, ["a", "b"], [1, 2])
    ops = SweepOps()
    rows = predict.run(predict_args("--multi_label", "brats", "--merge_type", "agg", *extra, src_list=lst, out_dir=out,
                                    patch_size="8,8,8", prep_mask="nonzero"), ops=ops, model=PointNet(), window_batch=3)
    with open(os.path.join(out, predict.PREDICT_CSV), newline="") as f:
        return rows, out, ops, list(csv.reader(f))


def test_predict_thresh_column_sits_after_blend_and_before_post(tmp_path, capsys):
    _, plain, _, t0 = _predict(tmp_path, "plain")
    assert t0[0] == predict.CSV_HEADER and "--thresh" not in capsys.readouterr().out
    _, moved, ops, t1 = _predict(tmp_path, "moved", "--thresh", "logit:0.125")
    said = capsys.readouterr().out
    assert t1[0] == predict.CSV_HEADER + ["thresh"] == predict.CSV_HEADER + predict.CSV_THRESH_COLUMNS
    assert [r[-1] for r in t1[1:]] == ["0.125", "0.125"] and [r[:12] for r in t1[1:]] == [r[:12] for r in t0[1:]]
    assert len([ln for ln in said.splitlines() if "[predict] --thresh" in ln and "0.125" in ln]) == 1
    assert ops.sigmoid_threshold() == 0.0                                     # the run restored the default
    a0 = nifti.read_nifti(os.path.join(plain, "a.nii.gz"))[0]
    a1 = nifti.read_nifti(os.path.join(moved, "a.nii.gz"))[0]
    assert (a0 != a1).any() and int((a1 > 0).sum()) < int((a0 > 0).sum())      # a higher threshold claims less
    _, _, _, t2 = _predict(tmp_path, "all", "--blend", "gauss", "--thresh", "0.75", "--post", "1:largest")
    assert t2[0] == predict.CSV_HEADER + ["blend", "tta_mirror", "thresh", "post", "post_changed"]
    assert t2[1][-3] == "%.9g" % np.float32(math.log(3.0)) and np.float32(float(t2[1][-3])) == np.float32(math.log(3.0))
    _, _, _, t3 = _predict(tmp_path, "post", "--thresh", "0.75", "--post", "1:largest")
    assert t3[0] == predict.CSV_HEADER + ["thresh", "post", "post_changed"]
    # 0.5 and logit:0 are the default: the file and the maps are byte for byte what they are without the switch
    capsys.readouterr()
    for k, value in enumerate(("0.5", "logit:0")):
        _, same, _, _ = _predict(tmp_path, f"same{k}", "--thresh", value)
        assert open(os.path.join(plain, "predict.csv"), "rb").read() == open(os.path.join(same, "predict.csv"), "rb").read()
        assert np.array_equal(nifti.read_nifti(os.path.join(same, "b.nii.gz"))[0],
                              nifti.read_nifti(os.path.join(plain, "b.nii.gz"))[0])
    assert "--thresh" not in capsys.readouterr().out


def test_predict_refuses_thresh_before_out_dir_exists(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst, _ = write_cases(root, ["a"], [1])
    for over, named in ((dict(thresh="0.3"), ["--thresh", "--multi_label"]),
                        (dict(thresh="2", multi_label="brats"), ["--thresh", "between 0 and 1"]),
                        (dict(thr_sweep=True), ["--thr_sweep", "predict"])):
        with pytest.raises(SystemExit) as e:
            predict.run(predict_args(src_list=lst, out_dir=out, patch_size="8,8,8", **over), ops=SweepOps(),
                        model=PointNet(), window_batch=2)
        assert all(n in str(e.value) for n in named), str(e.value)
        assert not os.path.exists(out)
