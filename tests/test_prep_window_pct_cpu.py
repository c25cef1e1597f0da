"""The percentile window of the `prep` mission (--prep_window pLO,pHI) without a device: the switch, the host half of
the rule, and the mission on the numpy stand-in of test_prep_cpu.py with the two new ops added."""
import csv
import os

import numpy as np
import pytest
import torch

from efficientq_amd import config as Cf, data as D, prep
from tests import prep_window_ref as Q
from tests import test_prep_cpu as R

MODS = D.MODALITIES["brats"]


class PctOps(R.NumpyOps):
    """... with prep_quantiles and prep_window_mask, from the restatement, and a count of their calls."""

    def __init__(self):
        self.calls = []

    def prep_quantiles(self, x, qs, mask="nonzero"):
        self.calls.append("quantiles")
        a = x.numpy()
        got = [Q.ref_stats(a[c], qs, mask) for c in range(a.shape[0])]
        return torch.tensor([n for n, _ in got]), torch.from_numpy(np.stack([s for _, s in got]))

    def prep_window_mask(self, x, lo, hi, mask="nonzero"):
        self.calls.append("window_mask")
        x.copy_(torch.from_numpy(Q.ref_window_mask(x.numpy(), lo, hi, mask)))
        return x


def run(root, out, window, ops=None, **over):
    args = R.prep_args(src_list=os.path.join(root, "cases.csv"), data_dir=out, prep_window=window, prep_min_size="4,4,4",
                       **over)
    return prep.run(args, ops=ops or PctOps())


# ---- the switch ---------------------------------------------------------------------------------------------------------
def test_parse_window_takes_the_percentile_form_and_keeps_the_old_forms(tmp_path):
    w = prep.parse_window("p0.5,p99.5", "brats")
    assert isinstance(w, prep.PercentileWindow) and (w.lo_q, w.hi_q) == (0.5, 99.5) and str(w) == "p0.5 p99.5"
    assert prep.parse_window(" P1 , p99 ", "lits") == prep.PercentileWindow(1.0, 99.0)
    assert prep.parse_window("p0,p100", "lits") == prep.PercentileWindow(0.0, 100.0)
    assert prep.parse_window(("p25", "p75"), "lits") == prep.PercentileWindow(25.0, 75.0)
    assert not isinstance(w, tuple) and w != (0.5, 99.5)
    # the old forms return what they returned
    assert prep.parse_window(None, "lits") == (-200.0, 250.0) and prep.parse_window(None, "brats") is None
    assert prep.parse_window("none", "lits") is None and prep.parse_window("", "lits") is None
    assert prep.parse_window("-5,7.5", "brats") == (-5.0, 7.5) and type(prep.parse_window("-5,7.5", "brats")) is tuple
    assert prep.parse_window((1, 2), "brats") == (1.0, 2.0)
    assert prep.WINDOW_DEFAULT == {"brats": None, "lits": (-200.0, 250.0)}
    # the command line and the YAML key
    a = Cf.build_parser().parse_args(["prep", "--task", "brats", "--prep_window", "p1,p99"])
    assert prep.parse_window(a.prep_window, "brats") == prep.PercentileWindow(1.0, 99.0)
    cfg = tmp_path / "p.yaml"
    cfg.write_text("prep_window: 'p2.5,p97.5'\n")
    a = Cf.merge_config(str(cfg), a)
    assert prep.parse_window(a.prep_window, "brats") == prep.PercentileWindow(2.5, 97.5)
    assert "pLO,pHI" in Cf.build_parser().format_help()


@pytest.mark.parametrize("text, why", [
    ("-200,p99", "one bound is a percentile and the other is not"),
    ("p1,250", "one bound is a percentile and the other is not"),
    ("p-1,p50", "a percentile lies within 0 and 100"),
    ("p1,p100.5", "a percentile lies within 0 and 100"),
    ("pnan,p50", "a percentile lies within 0 and 100"),
    ("p1,pinf", "a percentile lies within 0 and 100"),
    ("p50,p50", "pLO must lie below pHI"),
    ("p99,p1", "pLO must lie below pHI"),
    ("p1,p50,p99", "needs"),
    ("p1", "needs"),
    ("px,p99", "needs"),
    ("1,2,3", "needs"),
    ("low,high", "needs"),
])
def test_parse_window_refuses_by_name_and_names_the_three_forms(text, why):
    with pytest.raises(prep.PrepError) as e:
        prep.parse_window(text, "brats")
    said = str(e.value)
    assert f"--prep_window {text!r}" in said and why in said
    assert "lo,hi" in said and "pLO,pHI" in said and "none" in said


def test_a_bad_window_is_refused_before_anything_is_read_or_written(tmp_path):
    out = str(tmp_path / "out")
    args = R.prep_args(src_list=str(tmp_path / "missing.csv"), data_dir=out, prep_window="-200,p99")
    with pytest.raises(prep.PrepError, match="one bound is a percentile"):
        prep.run(args, ops=PctOps())
    assert not os.path.exists(out)
    with pytest.raises(prep.PrepError, match="lo must not exceed hi"):
        prep.parse_window("3,2", "brats")


# ---- the host half of the rule ---------------------------------------------------------------------------------------------
def test_percentile_value_is_the_rule_and_numpys_linear_method():
    g = np.random.default_rng(3)
    for n in (2, 3, 11, 1000):
        x = (500.0 * g.standard_normal(n)).astype(np.float32)
        s = np.sort(x)
        for q in (0.0, 0.5, 1.0, 37.5, 50.0, 99.5, 100.0, 100.0 * (n - 2) / (n - 1)):
            h, k = Q.ref_rank(n, q)
            a, b = s[k], s[min(k + 1, n - 1)]
            v = prep.percentile_value(n, q, a, b)
            assert isinstance(v, float) and np.float32(v) == v
            assert np.float32(v).view(np.uint32) == Q.ref_value(n, q, a, b).view(np.uint32)
            assert abs(v - np.percentile(x.astype(np.float64), q)) <= Q.percentile_bound(x, "all")
    assert prep.percentile_value(5, 100.0, 7.0, 7.0) == 7.0 and prep.percentile_value(5, 0.0, -3.0, 9.0) == -3.0
    assert prep.percentile_value(2, 50.0, -5.0, 5.0) == 0.0
    assert prep.percentile_value(3, 25.0, np.inf, np.inf) == np.inf             # a == b: no inf - inf
    assert np.isnan(prep.percentile_value(3, 25.0, -np.inf, 1.0)) or prep.percentile_value(3, 25.0, -np.inf, 1.0) == -np.inf
    assert np.isnan(prep.percentile_value(3, 25.0, 1.0, np.nan))


# ---- the mission on the numpy backend ---------------------------------------------------------------------------------------
def test_mission_clips_every_modality_to_its_own_percentiles_and_names_them(tmp_path, capsys):
    root = str(tmp_path)
    rows, truth = R.write_subjects(root, ["a", "b"], [1, 2])
    R.write_list(tmp_path / "cases.csv", rows)
    plain, out = os.path.join(root, "plain"), os.path.join(root, "out")
    run(root, plain, None)
    capsys.readouterr()
    ops = PctOps()
    got_rows = run(root, out, "p1,p99", ops=ops)
    said = capsys.readouterr().out
    assert ops.calls == (["quantiles"] + ["window_mask"] * 4) * 2
    table = list(csv.reader(open(os.path.join(out, prep.PREP_CSV))))
    cols = [f"{m}_win_{k}" for m in MODS for k in ("lo", "hi")]
    assert table[0] == prep.prep_csv_header(MODS) + cols and prep.window_columns(MODS) == cols
    old = list(csv.DictReader(open(os.path.join(plain, prep.PREP_CSV))))
    for line, before, row in zip(csv.DictReader(open(os.path.join(out, prep.PREP_CSV))), old, got_rows):
        sn = line["subject"]
        vols, seg, body = truth[sn]
        x = vols.astype(np.float32)
        assert line["pmin"] == before["pmin"] and line["pmax"] == before["pmax"]         # the crop box is what it was
        clipped = np.empty_like(x)
        for c, m in enumerate(MODS):
            lo, hi = float(line[f"{m}_win_lo"]), float(line[f"{m}_win_hi"])
            assert line[f"{m}_win_lo"] == repr(lo) == row[f"{m}_win_lo"] and line[f"{m}_win_hi"] == repr(hi)
            assert np.float32(lo) == lo and np.float32(hi) == hi
            inside = x[c][x[c] != 0].astype(np.float64)
            for q, v in ((1.0, lo), (99.0, hi)):
                assert np.float32(v).view(np.uint32) == Q.ref_percentile(x[c], q, "nonzero").view(np.uint32)
                assert abs(v - np.percentile(inside, q)) <= Q.percentile_bound(x[c], "nonzero")
            assert inside.min() < lo < hi < inside.max()                                 # the window clips something
            assert line[f"{m}_count"] == before[f"{m}_count"]
            assert f"{m} {lo:.7g} {hi:.7g}" in said
            clipped[c] = Q.ref_window_mask(x[c], lo, hi, "nonzero")
        assert f"[prep] {sn}: 20 24 28, window flair " in said
        _, count, total = R.ref_bbox_moments(clipped, "nonzero")
        mean = [s / n for s, n in zip(total, count)]
        std = [float(np.sqrt(v / n)) for v, n in zip(R.ref_sqdev(clipped, mean, "nonzero"), count)]
        pmin, pmax = tuple(s.start for s in body), tuple(s.stop for s in body)
        want = R.ref_standardise_crop(clipped, pmin, pmax, mean, std, "nonzero")
        for c, m in enumerate(MODS):
            arr = np.load(os.path.join(out, m, f"{sn}.npy"))
            assert np.array_equal(arr.view(np.uint32), want[c].view(np.uint32))
            assert np.array_equal(arr == 0, vols[c][body] == 0)                          # zeros stay zero, nothing else is
            assert not np.array_equal(arr, np.load(os.path.join(plain, m, f"{sn}.npy")))
            assert float(line[f"{m}_mean"]) == mean[c]
        assert np.array_equal(np.load(os.path.join(out, "seg", f"{sn}.npy")), seg[body])


def test_mask_all_counts_and_clips_every_voxel_and_cubic_reuses_the_bounds(tmp_path):
    root = str(tmp_path)
    rows, truth = R.write_subjects(root, ["a"], [4])
    R.write_list(tmp_path / "cases.csv", rows)
    out = os.path.join(root, "out")
    run(root, out, "p60,p90", prep_mask="all")
    line = list(csv.DictReader(open(os.path.join(out, prep.PREP_CSV))))[0]
    x = truth["a"][0].astype(np.float32)
    for c, m in enumerate(MODS):
        assert float(line[f"{m}_win_lo"]) == float(Q.ref_percentile(x[c], 60.0, "all")) > 0.0
        assert float(line[f"{m}_win_hi"]) == float(Q.ref_percentile(x[c], 90.0, "all"))
        arr = np.load(os.path.join(out, m, "a.npy"))
        assert len(np.unique(arr)) > 2 and arr.min() == arr[0, 0, 0]            # the zero margin went up to the low bound

    class Cubic(PctOps):
        """The cubic step stood in for by the trilinear one plus an overshoot that the second window has to clip."""

        def prep_resample_cubic(self, x, factors, out_shape, keep_zero=False):
            y = self.prep_resample(x, factors, out_shape)
            self.before = y.numpy().copy()
            y[:, 5, 5, 5] = 1e6
            return y

        def prep_standardise_crop(self, x, *a, **kw):
            self.seen = x.numpy().copy()
            return super().prep_standardise_crop(x, *a, **kw)

    ops = Cubic()
    out = os.path.join(root, "cubic")
    run(root, out, "p1,p99", ops=ops, prep_spacing="1,1,1", prep_interp="cubic")
    assert ops.calls == ["quantiles"] + ["window_mask"] * 8                      # found once, applied twice
    table = list(csv.reader(open(os.path.join(out, prep.PREP_CSV))))
    assert table[0][-9:] == ["interp"] + prep.window_columns(MODS)
    line = dict(zip(table[0], table[1]))
    for c, m in enumerate(MODS):
        hi = float(line[f"{m}_win_hi"])
        assert hi == float(Q.ref_percentile(x[c], 99.0, "nonzero")) and ops.seen[c, 5, 5, 5] == hi
        assert np.array_equal(ops.seen[c] == 0, ops.before[c] == 0)


# ---- the three stops ------------------------------------------------------------------------------------------------------
def _two_subjects_the_second_crafted(tmp_path, craft, dtype=np.int16):
    root = str(tmp_path)
    rows, truth = R.write_subjects(root, ["a", "b"], [1, 2])
    R.write_list(tmp_path / "cases.csv", rows)
    v = truth["b"][0][1].astype(dtype)          # t1 of subject b
    craft(v, truth["b"][2])
    R.write_scan(os.path.join(root, "src", "b_t1.nii.gz"), v)
    return root


def _stopped_at_b(root, window, named, **over):
    out = os.path.join(root, "out")
    with pytest.raises(prep.PrepError) as e:
        run(root, out, window, **over)
    said = str(e.value)
    assert "subject b" in said and "modality t1" in said and named in said, said
    files = R.written(out)
    assert files == sorted(f"{m}/a.npy" for m in list(MODS) + ["seg"])                 # nothing of b, none of the index files
    return said


def test_fewer_than_two_voxels_inside_the_mask_stop_the_run(tmp_path):
    def craft(v, body):
        v[...] = 0
        v[5, 6, 7] = 300
    said = _stopped_at_b(_two_subjects_the_second_crafted(tmp_path, craft), "p1,p99", "1 voxels inside the mask")
    assert "p1" in said and "p99" in said


def test_a_bound_that_is_not_finite_stops_the_run(tmp_path):
    def craft(v, body):
        v[body][:2] = np.inf
    root = _two_subjects_the_second_crafted(tmp_path, craft, np.float32)
    said = _stopped_at_b(root, "p1,p100", "the bound p100 of --prep_window is inf")
    assert "finite" in said


def test_a_bound_of_exactly_zero_under_nonzero_stops_the_run_and_under_all_does_not(tmp_path):
    def craft(v, body):
        n = v[body].size
        assert n % 2 == 0                       # h = (n - 1) / 2 lies half way between -5 and 5
        v[body] = np.where(np.arange(n) % 2 == 0, -5, 5).reshape(v[body].shape)
    root = _two_subjects_the_second_crafted(tmp_path, craft)
    said = _stopped_at_b(root, "p50,p100", "the bound p50 of --prep_window is exactly 0")
    assert "move voxels out of the mask" in said
    rows = run(root, os.path.join(root, "all"), "p50,p100", prep_mask="all")      # a bound of 0 under `all`: no voxel leaves
    assert [r["subject"] for r in rows] == ["a", "b"]


# ---- without the new form -------------------------------------------------------------------------------------------------
def test_an_absolute_window_writes_what_it_wrote_and_never_asks_for_a_percentile(tmp_path):
    root = str(tmp_path)
    rows, _ = R.write_subjects(root, ["a", "b"], [7, 8])
    R.write_list(tmp_path / "cases.csv", rows)
    ops = PctOps()
    new, old, none = (os.path.join(root, d) for d in ("new", "old", "none"))
    run(root, new, "300,2000", ops=ops)
    run(root, old, "300,2000", ops=R.NumpyOps())        # ops without the new methods: the path the parent took
    run(root, none, None, ops=ops)
    assert ops.calls == []
    assert R.written(new) == R.written(old) and prep.PREP_CSV in R.written(new)
    for f in R.written(new):
        assert open(os.path.join(new, f), "rb").read() == open(os.path.join(old, f), "rb").read(), f
    for d in (new, none):
        assert list(csv.reader(open(os.path.join(d, prep.PREP_CSV))))[0] == prep.prep_csv_header(MODS)
