"""effq_seg_sweep on a real MI355X (-m gpu): every histogram bit for bit against the numpy restatement
(tests/seg_sweep_ref.py, written from the definition), row 2048 and any other row against the decisions of
effq_seg_tallies, and --thr_sweep / --thresh end to end through the ptq and the predict mission.  Integers only."""
import csv
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, entrance, evaluate as E, nifti, predict, synth
from efficientq_amd.hip_ops import _ptr, get_ops
from tests import seg_sweep_ref as R
from tests.test_predict_cpu import ref_labels_source
from tests.test_predict_gpu import _scans
from tests.test_seg_eval_cpu import write_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = [1, 2, 3, 4, 8]
MODES = [("lits", None), ("brats", None), ("brats", "agg"), ("brats", "con")]
REF_MODE = {"lits": "argmax", "brats": "sigmoid"}
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


@pytest.fixture(scope="module")
def thresh(ops):
    t = ops.default_sigmoid_threshold()
    assert -2.0 ** -20 < t < 0.0              # about -1.78e-7: not 0, and inside (e_2047, e_2049)
    return t


def _labels(rng, task, Cc, S):
    if task == "lits":
        return rng.integers(0, Cc + 2, size=S).astype(np.uint8)            # values >= C belong to no class
    return (rng.random((Cc, S)) < 0.4).astype(np.uint8) * rng.integers(1, 256, size=(Cc, S)).astype(np.uint8)


def _run(ops, x, lab, task, fuse):
    got = ops.seg_sweep(torch.from_numpy(x).to(DEV), torch.from_numpy(lab).to(DEV), task, fuse)
    assert got.dtype == torch.int64 and tuple(got.shape) == (x.shape[0], 2, 4096)
    return got.cpu().numpy()


def _check(ops, thresh, x, lab, task, fuse, tag=""):
    """One call against the restatement, bit for bit; every class and truth sums to S."""
    x = np.ascontiguousarray(x, dtype=F32)
    got = _run(ops, x, lab, task, fuse)
    want = R.sweep(x, lab, REF_MODE[task], fuse, thresh)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{tag} {task}/{fuse} C {x.shape[0]} S {x.shape[1]}: first differences at (c, g, b) {bad[:5].tolist()}"
    assert (got.sum(axis=(1, 2)) == x.shape[1]).all()
    return got


def special_values(thresh):
    """Every e_k of k in {1, 2047, 2048, 2049, 4095} for both modes and the floats one ulp below and above, thresh and its
    neighbours, the zeros, the least subnormals, the infinities, NaN, values beyond +-16, and the float just under 1 / 128
    (where (s + 16) * 128 rounds up to 2049)."""
    inf = F32(np.inf)
    vals = []
    for e in (R.edges("sigmoid", thresh), R.edges("argmax")):
        for k in (1, 2047, 2048, 2049, 4095):
            vals += [e[k], np.nextafter(e[k], -inf), np.nextafter(e[k], inf)]
    t = F32(thresh)
    vals += [t, np.nextafter(t, -inf), np.nextafter(t, inf)]
    tiny = np.nextafter(F32(0), inf)
    vals += [F32(0.0), F32(-0.0), tiny, -tiny, inf, -inf, F32(np.nan), F32(16.5), F32(-16.5), F32(17.0), F32(-17.0),
             F32(1e30), F32(-1e30), F32(3.0e38), np.nextafter(F32(1.0 / 128.0), F32(0)), F32(15.999999), F32(-15.999999)]
    return np.array(vals, dtype=F32)


def _smallest_multi_trip_S(ops, Cc, task):
    """The least S at which a workgroup makes more than one trip, by bisection over the plan query."""
    lo, hi = 4, 8
    while ops.seg_sweep_plan(Cc, hi, task)["trips"] < 2:
        lo, hi = hi, hi * 2
        assert hi < 2 ** 30
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ops.seg_sweep_plan(Cc, mid, task)["trips"] >= 2 else (mid, hi)
    return hi


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task, fuse", MODES)
@pytest.mark.parametrize("Cc", CLASSES)
def test_shapes_with_tails_and_one_trip(ops, thresh, Cc, task, fuse):
    sv = special_values(thresh)
    for S in (1, 3, 4, 5, 255, 4099):
        rng = np.random.default_rng(1000 * Cc + S)
        x = (3.0 * rng.standard_normal((Cc, S))).astype(F32)
        sel = rng.random((Cc, S)) < 0.1
        x[sel] = rng.choice(sv, size=int(sel.sum()))
        plan = ops.seg_sweep_plan(Cc, S, task)
        assert plan["trips"] == (0 if S < 4 else 1) and plan["grid"] == (max(1, -(-(S // 4) // 512))) * ((Cc + 1) // 2)
        _check(ops, thresh, x, _labels(rng, task, Cc, S), task, fuse)


@pytest.mark.parametrize("task, fuse", MODES)
@pytest.mark.parametrize("Cc", CLASSES)
def test_several_trips_per_workgroup_with_a_tail(ops, thresh, Cc, task, fuse):
    S0 = _smallest_multi_trip_S(ops, Cc, task)
    assert ops.seg_sweep_plan(Cc, S0 - 1, task)["trips"] == 1 and S0 % 4 == 0
    S = S0 + 3
    assert ops.seg_sweep_plan(Cc, S, task)["trips"] == 2
    rng = np.random.default_rng(77 + Cc)
    x = (4.0 * rng.standard_normal((Cc, S))).astype(F32)
    x[:, rng.random(S) < 0.5] -= F32(25.0)                                  # half the voxels are background
    x[:, -3:] = F32(5.25)                                                   # the tail is seen: a bin nothing else is in
    _check(ops, thresh, x, _labels(rng, task, Cc, S), task, fuse)


# ---- edge values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task, fuse", MODES)
@pytest.mark.parametrize("Cc", CLASSES)
def test_edge_values_in_every_channel(ops, thresh, Cc, task, fuse):
    sv = special_values(thresh)
    n = len(sv)
    rng = np.random.default_rng(5 + Cc)
    blocks = []
    for c in range(Cc):                           # channel c walks the values, the others are ordinary
        b = rng.standard_normal((Cc, n)).astype(F32)
        b[c] = sv
        blocks.append(b)
        b = np.full((Cc, n), F32(-20.0))          # ... and are out of the way: the value decides alone
        b[c] = sv
        blocks.append(b)
    for shift in range(0, n, 7):                  # every channel walks them at once, each from another start
        blocks.append(np.stack([np.roll(sv, shift * (c + 1)) for c in range(Cc)]))
    if task == "lits" and Cc > 1:                 # margins that are edge values: x_0 - 0 with the other channels at 0
        b = np.zeros((Cc, n), dtype=F32)
        b[0] = sv
        blocks.append(b)
    x = np.concatenate(blocks, axis=1)
    got = _check(ops, thresh, x, _labels(rng, task, Cc, x.shape[1]), task, fuse)
    if task == "brats" and fuse is None:          # the restatement itself puts the named values where the issue says
        e = R.edges("sigmoid", thresh)
        assert R.bins_of(np.array([thresh, np.nextafter(F32(thresh), F32(-1)), np.nan, -np.inf, np.inf, 0.0, -0.0,
                                   np.nextafter(F32(1 / 128), F32(0)), 1 / 128], dtype=F32), e).tolist() == \
            [2048, 2047, 0, 0, 4095, 2048, 2048, 2048, 2049]
        assert got[:, :, 0].sum() > 0 and got[:, :, 4095].sum() > 0


# ---- argmax ties and NaN ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [2, 3, 4, 8])
def test_argmax_ties_nan_and_foreign_labels(ops, thresh, Cc):
    rng = np.random.default_rng(31 + Cc)
    cols = []
    for a in range(Cc):
        for b in range(a + 1, Cc):
            v = (rng.standard_normal(Cc) - 3.0).astype(F32)
            v[[a, b]] = F32(1.5)                                            # two equal maxima, margin exactly 0
            cols.append(v.copy())
            for c in range(b + 1, Cc):
                w = v.copy()
                w[c] = F32(1.5)                                             # three
                cols.append(w)
            w = v.copy()
            w[a] = F32(np.nan)                                              # NaN wins over the maximum
            cols.append(w)
            w = v.copy()
            w[[a, b]] = F32(np.nan)                                         # two NaN: the first wins, the second loses
            cols.append(w)
            w = (rng.standard_normal(Cc)).astype(F32)
            w[b] = F32(np.nan)
            w[a] = F32(np.inf)                                              # NaN beats +inf
            cols.append(w)
    cols.append(np.full(Cc, F32(np.inf)))                                   # inf - inf
    cols.append(np.full(Cc, F32(-np.inf)))
    cols.append(np.zeros(Cc, dtype=F32))
    cols.append(np.full(Cc, F32(np.nan)))
    x = np.stack(cols, axis=1)
    x = np.concatenate([x] * (Cc + 2), axis=1)                              # every column under every label value
    lab = np.repeat(np.arange(Cc + 2, dtype=np.uint8), len(cols))
    assert lab.max() >= Cc
    got = _check(ops, thresh, x, lab, "lits", None)
    win = R.torch_max_winner(x)
    # the pin: exactly one class per voxel is at or above 2048, torch.max's
    assert got[:, :, 2048:].sum() == x.shape[1]
    tw = torch.from_numpy(x).max(0)[1].numpy()                              # torch.max itself, NaN included
    assert np.array_equal(win, tw)
    assert [int(got[c, :, 2048:].sum()) for c in range(Cc)] == [int((tw == c).sum()) for c in range(Cc)]


# ---- contention -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task, Cc", [("brats", 2), ("lits", 3)])
def test_contention_from_one_bin_to_one_bin_per_lane(ops, thresh, task, Cc):
    S = 4 * 4096 + 2
    e = R.edges(REF_MODE[task], thresh)
    rng = np.random.default_rng(3)
    for n in (1, 2, 4, 5, 64):
        # lane l of a wave holds the voxels 4 l .. 4 l + 3 of its 256: (v // 4) % n gives the wave n distinct bins per add
        which = (np.arange(S) // 4) % n
        score = e[1000 + 37 * which].astype(F32) + F32(0.001)
        if task == "brats":
            x = np.stack([score, -score])
            lab = np.stack([np.ones(S, np.uint8), (which % 2).astype(np.uint8)])
        else:
            x = np.stack([score, np.zeros(S, F32), np.full(S, F32(-40.0))])  # margins: score, -score, far below
            lab = np.zeros(S, np.uint8) if n == 1 else (which % 3).astype(np.uint8)
        got = _check(ops, thresh, x, lab, task, None, f"n {n}")
        assert np.count_nonzero(got[0]) == n                                # n bins hold everything of class 0
        if n == 1:
            assert got[0].max() == S                                        # one bin, one truth
    # background-heavy: 97 % far below -16
    S = 300_001
    x = (2.0 * rng.standard_normal((Cc, S))).astype(F32)
    bg = rng.random(S) < 0.97
    x[:, bg] = F32(-30.0) if task == "brats" else x[:, bg]
    if task == "lits":
        x[0, bg] = F32(30.0)                                                # class 0 wins by far: margins beyond +-16
    lab = _labels(rng, task, Cc, S)
    if task == "brats":
        lab[:, bg] = 0
    else:
        lab[bg] = 0
    got = _check(ops, thresh, x, lab, task, None, "background")
    assert got[-1, 0, 0] >= 0.9 * S


# ---- rows are decisions -----------------------------------------------------------------------------------------------------
def _mixed(rng, Cc, S):
    x = np.round(2.0 * rng.standard_normal((Cc, S)), 1).astype(F32)         # one decimal: ties among the channels
    x[rng.random((Cc, S)) < 0.02] = F32(np.nan)
    x[rng.random((Cc, S)) < 0.02] = F32(0.0)
    x[rng.random((Cc, S)) < 0.01] = F32(-0.0)
    return x


@pytest.mark.parametrize("task, fuse", MODES)
@pytest.mark.parametrize("Cc", [1, 2, 3, 8])
def test_row_2048_is_the_decision_of_the_tallies(ops, thresh, Cc, task, fuse):
    S = 20_003
    rng = np.random.default_rng(900 + Cc)
    x = _mixed(rng, Cc, S)
    x[:, :3] = F32(thresh)
    x[:, 3:6] = np.nextafter(F32(thresh), F32(-1))
    lab = _labels(rng, task, Cc, S)
    got = _check(ops, thresh, x, lab, task, fuse)
    counts = ops.seg_tallies(torch.from_numpy(x).to(DEV), torch.from_numpy(lab).to(DEV), task, fuse).cpu().numpy()
    assert np.array_equal(R.decision_counts(got, 2048), counts)
    if task == "lits" and Cc > 1:
        assert np.isnan(x).any() and (np.sort(x, 0)[-1] == np.sort(x, 0)[-2]).sum() > 50      # NaN and ties were there


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
@pytest.mark.parametrize("Cc", [1, 3, 8])
def test_any_row_is_the_decision_at_its_edge(ops, thresh, Cc, fuse):
    S = 20_003
    rng = np.random.default_rng(400 + Cc)
    x = _mixed(rng, Cc, S)
    lab = _labels(rng, "brats", Cc, S)
    xd, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(lab).to(DEV)
    got = _check(ops, thresh, x, lab, "brats", fuse)
    edges = ops.sweep_edges("brats")
    assert np.array_equal(edges.numpy().view(np.int32), R.edges("sigmoid", thresh).view(np.int32))
    try:
        for k in (1, 1500, 1920, 2047, 2048, 2049, 2100, 2304, 4095):
            ops.set_decision_threshold(float(edges[k]))
            assert ops.sigmoid_threshold() == float(edges[k])
            counts = ops.seg_tallies(xd, ld, "brats", fuse).cpu().numpy()
            assert np.array_equal(R.decision_counts(got, k), counts), k
            again = ops.seg_sweep(xd, ld, "brats", fuse).cpu().numpy()      # the sweep keeps the default edge
            assert np.array_equal(again, got)
    finally:
        ops.set_decision_threshold(None)
    assert ops.sigmoid_threshold() == thresh


def test_equal_bits_on_every_call_and_a_garbage_hist_is_overwritten(ops, thresh):
    S, Cc = 50_003, 3
    rng = np.random.default_rng(8)
    x = _mixed(rng, Cc, S)
    for task in ("lits", "brats"):
        lab = _labels(rng, task, Cc, S)
        xd, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(lab).to(DEV)
        a = ops.seg_sweep(xd, ld, task)
        b = ops.seg_sweep(xd, ld, task)
        assert torch.equal(a, b)
        hist = torch.full((Cc, 2, 4096), -123456789012, dtype=torch.int64, device=DEV)
        mode = _lib.SEG_ARGMAX if task == "lits" else _lib.SEG_SIGMOID
        rc = ops.lib.effq_seg_sweep(_ptr(xd), _ptr(ld), Cc, S, mode, 0, thresh, _ptr(hist), ops.stream)
        assert rc == 0 and torch.equal(hist, a)
        # refused before any launch: hist stays what it was
        hist.fill_(7)
        assert ops.lib.effq_seg_sweep(_ptr(xd), _ptr(ld), Cc, S, mode, 0, 0.5, _ptr(hist), ops.stream) == \
            (1 if task == "brats" else 0)
        assert ops.lib.effq_seg_sweep(_ptr(xd), _ptr(ld), 9, S, mode, 0, thresh, _ptr(hist), ops.stream) == 1
        torch.cuda.synchronize()
        if task == "brats":
            assert int(hist.min()) == 7 and int(hist.max()) == 7
    with pytest.raises(_lib.EffqError):
        ops.seg_sweep(torch.from_numpy(x).to(DEV), torch.zeros(S, dtype=torch.uint8, device=DEV), "lits", "agg")


# ---- end to end: the ptq mission ---------------------------------------------------------------------------------------------
def _ptq(tmp_path, name, task, data_dir, split_dir, *extra):
    snap = str(tmp_path / name)
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--patch_size", "20,20,18", "--data_dir", data_dir,
            "--split_dir", split_dir, "--test_fp", "--snap_dir", snap]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", "agg"]
    entrance.main(argv + list(extra))
    return snap


def _table(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


@pytest.mark.parametrize("task", ["lits", "brats"])
def test_ptq_mission_sweeps_both_networks_and_thresh_reaches_the_best_row(tmp_path, monkeypatch, capsys, task):
    shape = (20, 24, 18)
    data_dir, split_dir, _ = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy", train=["c2", "c0"],
                                           val=["c1", "c0"])
    seen = []
    whole = E.validate_seg

    def spy(*a, **k):
        res = whole(*a, **k)
        seen.append(res)
        return res
    monkeypatch.setattr(E, "validate_seg", spy)
    snap = _ptq(tmp_path, "sweep", task, data_dir, split_dir, "--thr_sweep")
    said = capsys.readouterr().out
    assert "--thr_sweep" in said and "FP: AUC" in said and "PTQ: AUC" in said
    assert len([ln for ln in said.splitlines() if "FP: AUC" in ln and "PTQ: AUC" in ln]) == 3      # side by side, per class
    assert len(seen) == 2
    ncls = 3
    pooled_best = {}
    for folder, res in zip(("fp", "ptq"), seen):
        out = os.path.join(snap, folder)
        assert sorted(os.listdir(out)) == ["metrics.csv", "threshold.csv", "threshold_curve.csv"]
        thr, curve, met = (_table(os.path.join(out, f)) for f in ("threshold.csv", "threshold_curve.csv", "metrics.csv"))
        assert tuple(thr[0]) == E.THRESHOLD_COLUMNS and tuple(curve[0]) == E.THRESHOLD_CURVE_COLUMNS
        assert [(r[0], r[1]) for r in thr[1:]] == [(s, str(c)) for s in ("c0", "c1", "pooled") for c in range(ncls)]
        assert len(curve) == 1 + ncls * 4095
        edges = res[0]["sweep_edges"]
        want = E.sweep_summary(E.sweep_pooled([r["sweep"] for r in res]), edges)
        for c, row in enumerate(r for r in thr[1:] if r[0] == "pooled"):
            q = want[c]
            assert row[2] == "%.9g" % q["auc"] and row[3] == "%.7g" % float(q["dsc_default"])
            assert float(row[4]) == q["best_thr"] and row[6] == "%.7g" % float(q["dsc_best"])
            assert [int(v) for v in row[9:]] == [q["pos"], q["neg"]] and q["pos"] + q["neg"] == 2 * int(np.prod(shape))
            assert float(q["dsc_best"]) >= float(q["dsc_default"])
            crow = curve[1 + c * 4095 + q["best_k"] - 1]
            assert crow[:2] == [str(c), str(q["best_k"])] and float(crow[2]) == q["best_thr"]
            assert [int(v) for v in crow[4:8]] == q["counts"][q["best_k"]].tolist()
            pooled_best[(folder, c)] = (row[4], [int(v) for v in crow[4:8]])
        for r in res:                        # the sweep is the restatement's, and its row 2048 is metrics.csv's
            assert np.array_equal(R.decision_counts(r["sweep"].numpy(), 2048), r["counts"].numpy())
        dsc = {(r[0], r[1]): r[2] for r in met[1:]}
        assert {(r[0], r[1]): r[3] for r in thr[1:] if r[0] != "pooled"} == dsc
    if task == "lits":
        with pytest.raises(SystemExit) as e:
            _ptq(tmp_path, "refused", task, data_dir, split_dir, "--thresh", "0.3")
        assert "--thresh" in str(e.value) and "--multi_label" in str(e.value) and not os.path.exists(str(tmp_path / "refused"))
        return
    # the same run decided at the pooled best threshold of class 1 of the calibrated network: metrics.csv's counts of that
    # class, summed over the subjects, are the curve's row
    logit, counts = pooled_best[("ptq", 1)]
    assert float(logit) != 0.0
    snap2 = _ptq(tmp_path, "thresh", task, data_dir, split_dir, "--thresh", f"logit:{logit}")
    said = capsys.readouterr().out
    assert len([ln for ln in said.splitlines() if "[entrance] --thresh" in ln and f"{float(logit):.9g}" in ln]) == 1
    met = _table(os.path.join(snap2, "ptq", "metrics.csv"))
    got = np.sum([[int(v) for v in r[6:10]] for r in met[1:] if r[1] == "1"], axis=0)
    assert got.tolist() == counts
    assert sorted(os.listdir(os.path.join(snap2, "ptq"))) == ["metrics.csv"]
    fp_at = E.sweep_summary(E.sweep_pooled([r["sweep"] for r in seen[0]]), seen[0][0]["sweep_edges"])[1]
    k = int(np.searchsorted(seen[0][0]["sweep_edges"].numpy()[1:], np.float32(float(logit)), side="right"))
    met_fp = _table(os.path.join(snap2, "fp", "metrics.csv"))
    got_fp = np.sum([[int(v) for v in r[6:10]] for r in met_fp[1:] if r[1] == "1"], axis=0)
    assert got_fp.tolist() == fp_at["counts"][k].tolist()                  # the FP network is decided there too
    assert get_ops(DEV).sigmoid_threshold() == get_ops(DEV).default_sigmoid_threshold()    # the run restored the default


# ---- end to end: predict --thresh ---------------------------------------------------------------------------------------------
def test_predict_thresh_moves_exactly_the_voxels_between_the_two_thresholds(ops, thresh, tmp_path, monkeypatch):
    root = str(tmp_path)
    lst = _scans(root, ["b", "a"])
    args = Cf.make_args(dict(Cf.TINY_NET, qconv="conv", nClass=4, multi_label="brats"), 4, 4, merge_type="agg")
    QConv, _, kwQ = Cf.get_conv_class(args)
    net = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(net, 0)
    ckpt = os.path.join(root, "state.pkl")
    torch.save({"state_dict": net.state_dict()}, ckpt)
    calls = []
    whole = ops.seg_labels_source

    def spy(logits, pmin, grid, factors, source_shape, rule, fuse=None):
        calls.append((logits.cpu().numpy(), tuple(pmin), tuple(grid), factors, tuple(source_shape), rule, fuse))
        return whole(logits, pmin, grid, factors, source_shape, rule, fuse)
    monkeypatch.setattr(ops, "seg_labels_source", spy)

    def run(name, value):
        for k, v in dict(src_list=lst, out_dir=os.path.join(root, name), patch_size="32,32,32", prep_mask="nonzero",
                         pretrain=ckpt, thresh=value, mission="predict").items():
            setattr(args, k, v)
        predict.run(args, window_batch=1)
        return _table(os.path.join(root, name, predict.PREDICT_CSV))
    t0 = run("plain", None)
    assert t0[0] == predict.CSV_HEADER and len(calls) == 2
    ch0 = np.concatenate([c[0][0].ravel() for c in calls])
    t1 = float(np.float32(np.quantile(ch0, 0.6)))
    assert abs(t1) > 1e-3
    first = list(calls)
    t2 = run("moved", f"logit:{t1:.9g}")
    assert t2[0] == predict.CSV_HEADER + ["thresh"] and [r[-1] for r in t2[1:]] == ["%.9g" % t1] * 2
    assert [r[:12] for r in t2[1:]] == [r[:12] for r in t0[1:]]
    assert ops.sigmoid_threshold() == thresh                                # restored
    t3 = run("same", "0.5")
    assert t3 == t0                                                         # 0.5 is the default: nothing changes
    for f in ("a.nii.gz", "b.nii.gz"):
        a, b = (nifti.read_nifti(os.path.join(root, d, f))[0] for d in ("plain", "same"))
        assert a.tobytes() == b.tobytes()
    a, b = (open(os.path.join(root, d, predict.PREDICT_CSV), "rb").read() for d in ("plain", "same"))
    assert a == b
    moved = 0
    lo, hi = min(thresh, t1), max(thresh, t1)
    for sn, (logits, pmin, grid, factors, source, rule, fuse), again in zip(("a", "b"), first, calls[2:4]):
        assert np.array_equal(logits, again[0]) and (rule, fuse) == ("brats", "agg")
        m0 = nifti.read_nifti(os.path.join(root, "plain", f"{sn}.nii.gz"))[0]
        m1 = nifti.read_nifti(os.path.join(root, "moved", f"{sn}.nii.gz"))[0]
        w0, _, inside = ref_labels_source(logits, pmin, grid, factors, source, rule, fuse, thresh)
        w1, _, _ = ref_labels_source(logits, pmin, grid, factors, source, rule, fuse, t1)
        assert factors is None or tuple(factors) == (1.0, 1.0, 1.0)         # no resampling: the recount is exact
        assert np.array_equal(m0, w0) and np.array_equal(m1, w1)
        # a voxel of the box changes its merged planes exactly when one of its logits lies between the two thresholds
        between = ((logits >= lo) & (logits < hi)).any(0)
        box = tuple(slice(a, a + n) for a, n in zip(pmin, logits.shape[1:]))
        planes0 = R.scores(logits.reshape(3, -1), "sigmoid", "agg") >= np.float32(thresh)
        planes1 = R.scores(logits.reshape(3, -1), "sigmoid", "agg") >= np.float32(t1)
        changed = (planes0 != planes1).any(0).reshape(logits.shape[1:])
        assert not changed[~between].any() and changed.any()
        assert np.array_equal((m0 != m1)[box] & ~changed, np.zeros_like(changed))
        assert not (m0 != m1)[~inside].any()
        moved += int((m0 != m1).sum())
    assert moved > 0, "the threshold moved no voxel: the test shows nothing"
