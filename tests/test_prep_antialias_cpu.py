"""`--prep_antialias`, host side (no GPU): the restatement tests/prep_smooth_ref.py against scipy and a closed form, the
rule of sigma, radius and taps (prep.antialias_*), the switch and its refusals, the C-ABI row of effq_prep_smooth, and
the `prep` and `predict` missions driven through numpy stand-ins that add prep_smooth."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, data as D, predict, prep
from tests import prep_smooth_ref as S
from tests.test_predict_cpu import PointNet, predict_args, write_cases
from tests.test_prep_cpu import NumpyOps, prep_args, write_list, write_subjects, written
from tests.test_window_blend_cpu import BlendOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = {0.5: (0.0, 0), 1.0: (0.0, 0), 1.4: (0.2, 1), 2.0: (0.5, 2), 2.5: (0.75, 3), 17.0: (8.0, 32)}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_equals_scipy_per_axis():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in ((2, 7, 9, 11), (1, 2, 2, 2)):                 # the second: every extent below the radius of 3
        x = np.random.default_rng(0).standard_normal(shape)
        for sigma in (0.2, 0.5, 0.75, 8.0):
            for a, axis in enumerate((-3, -2, -1)):
                sig = [0.0, 0.0, 0.0]
                sig[a] = sigma
                got = S.ref_smooth(x, sig, rounded=False)
                want = ndi.gaussian_filter1d(x, sigma, axis=axis, mode="nearest", truncate=4.0)
                assert np.abs(got - want).max() <= 1e-13, (shape, sigma, axis)
    # the three axes one after the other are scipy's three calls, W then H then D
    x = np.random.default_rng(1).standard_normal((7, 9, 11))
    want = x
    for axis, sigma in ((2, 0.5), (1, 0.2), (0, 0.75)):
        want = ndi.gaussian_filter1d(want, sigma, axis=axis, mode="nearest", truncate=4.0)
    assert np.abs(S.ref_smooth(x, (0.75, 0.2, 0.5), rounded=False) - want).max() <= 1e-13


@pytest.mark.parametrize("factor", list(FACTORS))
def test_sigma_radius_and_taps_follow_the_rule(factor):
    sigma, r = FACTORS[factor]
    assert prep.antialias_sigma(factor) == pytest.approx(sigma, abs=1e-15) == pytest.approx(S.ref_sigma(factor), abs=1e-15)
    sigma = prep.antialias_sigma(factor)
    assert prep.antialias_radius(sigma) == r == S.ref_radius(sigma)
    taps = prep.antialias_taps(sigma)
    assert taps.dtype == np.float32 and taps.shape == (r + 1,) and taps.flags["C_CONTIGUOUS"]
    if r == 0:
        assert taps.tolist() == [1.0]
        return
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * sigma * sigma))
    g /= g.sum()
    assert abs(g.sum() - 1.0) <= 1e-15
    assert np.array_equal(taps, g[r:].astype(np.float32))                  # centre first, rounded once, bit for bit
    assert np.array_equal(S.ref_taps(sigma)[r:], taps.astype(np.float64))
    full = np.concatenate([taps[:0:-1], taps]).astype(np.float64)
    assert abs(full.sum() - 1.0) <= (2 * r + 1) * 2.0 ** -24               # not normalised again after the rounding
    assert np.all(taps > 0) and np.all(np.diff(taps) < 0)
    if factor == 2.0:                                                       # sigma 0.5: 1, e^-2, e^-8 over their sum
        e2, e8 = np.exp(-2.0), np.exp(-8.0)
        assert taps.astype(np.float64) == pytest.approx(np.array([1.0, e2, e8]) / (1 + 2 * e2 + 2 * e8), rel=2.0 ** -24)


def test_radius_cap_is_the_headers_and_the_libs():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    cap = int(re.search(r"#define EFFQ_PREP_SMOOTH_MAX_RADIUS (\d+)", hdr).group(1))
    assert cap == 32 == _lib.PREP_SMOOTH_MAX_RADIUS == prep.ANTIALIAS_MAX_RADIUS == S.MAX_RADIUS
    assert prep.antialias_radius(prep.antialias_sigma(17.0)) == cap
    assert prep.antialias_radius(prep.antialias_sigma(17.3)) > cap


def test_stripes_keep_the_closed_form_amplitude():
    sigma = prep.antialias_sigma(2.5)
    g = S.ref_taps(sigma, rounded=False)
    r = (len(g) - 1) // 2
    amp = float(sum(g[k + r] * (-1.0) ** k for k in range(-r, r + 1)))
    assert amp == pytest.approx(0.125, abs=0.01)
    n = 16
    for a in range(3):
        shape = [5, 6, 7]
        shape[a] = n
        idx = np.arange(n).reshape([-1 if b == a else 1 for b in range(3)])
        x = np.broadcast_to((-1.0) ** idx, shape)
        sig = [0.0, 0.0, 0.0]
        sig[a] = sigma
        y = S.ref_smooth(x, sig, rounded=False)
        inner = np.take(y, np.arange(r, n - r), axis=a), np.take(x, np.arange(r, n - r), axis=a)
        assert np.abs(inner[0] - amp * inner[1]).max() <= 1e-12
    assert np.array_equal(S.ref_smooth(np.zeros((3, 4, 5)), (0.75, 0.75, 0.75)), np.zeros((3, 4, 5)))
    # keep_zero: exactly zero where the input is, the rest untouched
    x = np.random.default_rng(2).standard_normal((6, 7, 8))
    x[2:4, :, 3:5] = 0.0
    y0, y1 = S.ref_smooth(x, (0.75, 0.2, 0.5)), S.ref_smooth(x, (0.75, 0.2, 0.5), keep_zero=True)
    assert np.all(y1[x == 0] == 0) and np.all(y0[x == 0] != 0) and np.array_equal(y1[x != 0], y0[x != 0])


# ---- the symbol ----------------------------------------------------------------------------------------------------------
def test_smooth_symbol_in_header_lib_and_makefile():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.findall(r"\bint (effq_prep_smooth)\s*\((.*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _lib._P
        return {"int": _lib._I, "float": _lib._F, "double": _lib._D, "size_t": _lib._SZ}[decl.split()[0]]
    args = [a.strip() for a in found[0][1].split(",")]
    res, got = _lib.SIGNATURES["effq_prep_smooth"]
    assert res == _lib._I and got == [ctype(a) for a in args]
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["x", "N", "D", "H", "W", "taps_d", "rd", "taps_h", "rh", "taps_w", "rw", "keep_zero", "y", "tmp", "stream"]
    make = open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "prep_smooth.hip" in srcs and "prep.hip" in srcs
    deps = re.search(r"^%\.o: (.*)$", make, flags=re.M).group(1).split()
    src = open(os.path.join(ROOT, "efficientq_amd", "csrc", "prep_smooth.hip")).read()
    for inc in re.findall(r'#include "([^"]+)"', src):
        assert inc in deps, inc
    assert not re.search(r"atomic\w*\s*\(", re.sub(r"//.*", "", src))       # deterministic: no atomics at all
    assert not re.search(r"hipMalloc|hipMemcpy|hipFree", src)               # the taps travel in the launch parameters


# ---- the switch ----------------------------------------------------------------------------------------------------------
def test_parser_knows_the_switch_and_yaml_sets_it(tmp_path):
    for mission in ("prep", "predict", "ptq"):
        assert Cf.build_parser().parse_args([mission]).prep_antialias is False
        assert Cf.build_parser().parse_args([mission, "--prep_antialias"]).prep_antialias is True
    cfg = tmp_path / "p.yaml"
    cfg.write_text("prep_antialias: true\nprep_spacing: '2,2,2'\n")
    a = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["prep"]))
    assert a.prep_antialias is True and prep.antialias_switch(a, (2.0, 2.0, 2.0)) is True
    assert prep.antialias_switch(Cf.build_parser().parse_args(["prep"]), None) is False


class SmoothMixin:
    """prep_smooth through the restatement, with a record of the calls."""

    def prep_smooth(self, x, sigmas, keep_zero=False):
        if not hasattr(self, "smoothed"):
            self.smoothed = []
        self.smoothed.append((tuple(x.shape), str(x.dtype), tuple(float(s) for s in sigmas), bool(keep_zero)))
        assert any(S.ref_radius(s) > 0 for s in sigmas)                    # the mission calls only when there is work
        return torch.from_numpy(S.ref_smooth(x.numpy(), sigmas, keep_zero).astype(np.float32))


class SmoothNumpyOps(SmoothMixin, NumpyOps):
    pass


class SmoothPredictOps(SmoothMixin, BlendOps):
    pass


def test_refused_without_a_spacing_and_beyond_the_radius_cap_before_anything_is_written(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "out")
    rows, _ = write_subjects(root, ["a", "b"], [1, 2], affine=np.diag([1.0, 1.0, 0.1, 1.0]))
    lst = write_list(tmp_path / "cases.csv", rows)
    cases, _ = write_cases(os.path.join(root, "ct"), ["a", "b"], [1, 2], affine=np.diag([1.0, 1.0, 0.1, 1.0]))

    def refused(named, **over):
        for run in (lambda: prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="1,1,1", prep_antialias=True,
                                               **over), ops=SmoothNumpyOps()),
                    lambda: predict.run(predict_args(src_list=cases, out_dir=out, patch_size="1,1,1",
                                                     prep_antialias=True, **over), ops=SmoothPredictOps(),
                                        model=PointNet(), window_batch=2)):
            with pytest.raises(SystemExit) as e:
                run()
            assert isinstance(e.value, prep.PrepError) and all(n in str(e.value) for n in named), str(e.value)
            assert not os.path.exists(out)
    refused(["--prep_antialias", "--prep_spacing"])
    # 0.1 mm to 1.73 mm: a factor of 17.3 along array axis 2, a radius of 33
    refused(["subject a", "--prep_antialias", "axis 2", "17.3", "33"], prep_spacing="1,1,1.73")
    # a factor of 17 is the last that fits
    plan = prep._Plan(prep.read_src_list(lst, "brats")[0], D.MODALITIES["brats"], (1.0, 1.0, 1.7), (1, 1, 1), None, True)
    assert plan.radii == (0, 0, 32) and plan.sigmas == pytest.approx((0.0, 0.0, 8.0))


# ---- the missions on the host --------------------------------------------------------------------------------------------
def _table(path):
    return list(csv.reader(open(path)))


def _arrays(root):
    return {f: open(os.path.join(root, f), "rb").read() for f in written(root) if f.endswith(".npy")}


def test_prep_mission_filters_before_the_resample_and_records_the_sigmas(tmp_path, capsys):
    root = str(tmp_path)
    mods = D.MODALITIES["brats"]
    rows, truth = write_subjects(root, ["a"], [5], affine=np.eye(4))
    lst = write_list(tmp_path / "cases.csv", rows)
    kw = dict(prep_spacing="2.5,1.4,1", prep_min_size="4,4,4")
    # without the switch: a stand-in that has no prep_smooth does, and every file is what a stand-in with one writes
    off, off2 = os.path.join(root, "off"), os.path.join(root, "off2")
    prep.run(prep_args(src_list=lst, data_dir=off, **kw), ops=NumpyOps())
    said_off = capsys.readouterr().out
    ops = SmoothNumpyOps()
    prep.run(prep_args(src_list=lst, data_dir=off2, **kw), ops=ops)
    assert not hasattr(ops, "smoothed") and capsys.readouterr().out == said_off.replace(off, off2)
    assert "anti-alias" not in said_off
    assert _table(os.path.join(off, prep.PREP_CSV))[0] == prep.prep_csv_header(mods)
    assert written(off) == written(off2)
    for f in written(off):
        if not f.endswith(".gz") and f != D.SN_FN_FILE:          # gzip stamps the time
            assert open(os.path.join(off, f), "rb").read() == open(os.path.join(off2, f), "rb").read(), f

    # with it: one call per subject on the four modalities, never on the label; mask nonzero keeps the zeros
    on = os.path.join(root, "on")
    ops = SmoothNumpyOps()
    got = prep.run(prep_args(src_list=lst, data_dir=on, prep_antialias=True, **kw), ops=ops)
    said = capsys.readouterr().out
    assert ops.smoothed == [((4, 20, 24, 28), "torch.float32", pytest.approx((0.75, 0.2, 0.0)), True)]
    assert "a: 20 24 28, anti-alias sigma 0.75 0.2 0 -> " in said
    t_on, t_off = _table(os.path.join(on, prep.PREP_CSV)), _table(os.path.join(off, prep.PREP_CSV))
    assert t_on[0] == prep.prep_csv_header(mods) + ["antialias"] and t_on[1][-1] == "0.75 0.2 0" == got[0]["antialias"]
    r_on, r_off = dict(zip(t_on[0], t_on[1])), dict(zip(t_off[0], t_off[1]))
    assert (r_on["pmin"], r_on["pmax"], r_on["grid_shape"]) == (r_off["pmin"], r_off["pmax"], r_off["grid_shape"])
    assert r_on["flair_count"] == r_off["flair_count"] and r_on["flair_std"] != r_off["flair_std"]
    for m in mods:
        a, b = np.load(os.path.join(on, m, "a.npy")), np.load(os.path.join(off, m, "a.npy"))
        assert a.shape == b.shape and np.array_equal(a == 0, b == 0) and not np.array_equal(a, b)
        assert np.all(a.view(np.uint32)[a == 0] == 0)                      # +0.0f
    assert open(os.path.join(on, "seg", "a.npy"), "rb").read() == open(os.path.join(off, "seg", "a.npy"), "rb").read()
    # the arrays are the numpy pipeline's: window (none for brats), filter, resample, standardise
    vols = truth["a"][0].astype(np.float32)
    sm = S.ref_smooth(vols, (0.75, 0.2, 0.0), keep_zero=True).astype(np.float32)
    assert np.all(sm[vols == 0] == 0) and np.all(sm[vols != 0] != 0)
    want = prep.process_subject(NumpyOps(), prep._Plan(prep.read_src_list(lst, "brats")[0], mods, (2.5, 1.4, 1.0), (4, 4, 4)),
                                dict(zip(mods, sm)), None, mods,
                                prep.PrepOptions("nonzero", None, (2.5, 1.4, 1.0), (4, 4, 4), False))[0]
    assert np.array_equal(np.stack([np.load(os.path.join(on, m, "a.npy")) for m in mods]), want)

    # a second run into the same folder merges: a subject that is only kept or up-sampled gets 0 0 0, the op is not called
    rows2, _ = write_subjects(os.path.join(root, "more"), ["b"], [6], affine=np.diag([3.0, 2.0, 1.0, 1.0]))
    lst2 = write_list(os.path.join(root, "more", "cases.csv"), rows2)
    ops = SmoothNumpyOps()
    prep.run(prep_args(src_list=lst2, data_dir=on, prep_antialias=True, **kw), ops=ops)
    said = capsys.readouterr().out
    assert not hasattr(ops, "smoothed") and "anti-alias" not in said
    t2 = _table(os.path.join(on, prep.PREP_CSV))
    assert t2[0] == t_on[0] and [r[0] for r in t2[1:]] == ["a", "b"] and t2[1] == t_on[1] and t2[2][-1] == "0 0 0"
    # with --prep_orient the column still comes last
    both = os.path.join(root, "both")
    prep.run(prep_args(src_list=lst, data_dir=both, prep_antialias=True, prep_orient="RAS", **kw), ops=SmoothNumpyOps())
    t3 = _table(os.path.join(both, prep.PREP_CSV))
    assert t3[0] == prep.prep_csv_header(mods) + prep.ORIENT_COLUMNS + ["antialias"] and t3[1][-3:] == ["RAS", "RAS", "0.75 0.2 0"]
    # into a folder whose prep.csv is older than the column: the table takes the new header, as with the orient columns,
    # and stays rectangular
    prep.run(prep_args(src_list=lst2, data_dir=off, prep_antialias=True, **kw), ops=SmoothNumpyOps())
    t4 = _table(os.path.join(off, prep.PREP_CSV))
    assert t4[0] == t_on[0] and all(len(r) == len(t4[0]) for r in t4) and t4[-1][0] == "b" and t4[-1][-1] == "0 0 0"


def test_predict_mission_filters_as_prep_does_and_records_the_sigmas(tmp_path, capsys):
    root = str(tmp_path)
    lst, truth = write_cases(root, ["s1", "s2"], [3, 4], affine=np.diag([1.0, 1.0, 2.0, 1.0]))
    kw = dict(src_list=lst, patch_size="8,8,8", prep_spacing="2.5,1.4,2", prep_mask="nonzero")

    def run(name, ops, *extra, **over):
        out = os.path.join(root, name)
        rows = predict.run(predict_args(*extra, out_dir=out, **dict(kw, **over)), ops=ops, model=PointNet(), window_batch=3)
        return out, rows, _table(os.path.join(out, predict.PREDICT_CSV)), capsys.readouterr().out
    off, _, t_off, said_off = run("off", BlendOps())
    ops = SmoothPredictOps()
    off2, _, t_off2, said_off2 = run("off2", ops)
    assert not hasattr(ops, "smoothed") and t_off == t_off2 and t_off[0] == predict.CSV_HEADER
    assert said_off2 == said_off.replace(off, off2) and "anti-alias" not in said_off
    assert open(os.path.join(off, predict.PREDICT_CSV), "rb").read() == open(os.path.join(off2, predict.PREDICT_CSV), "rb").read()

    ops = SmoothPredictOps()
    on, rows, t_on, said = run("on", ops, "--prep_antialias")
    assert ops.smoothed == [((1, 20, 24, 28), "torch.float32", pytest.approx((0.75, 0.2, 0.0)), True)] * 2
    assert t_on[0] == predict.CSV_HEADER + ["antialias"] and [r[-1] for r in t_on[1:]] == ["0.75 0.2 0"] * 2
    assert rows[0]["antialias"] == "0.75 0.2 0" and said.count(", anti-alias sigma 0.75 0.2 0 -> grid 8 17 28") == 2
    assert [r[:len(predict.CSV_HEADER)][:7] for r in t_on[1:]] == [r[:7] for r in t_off[1:]]      # the grid and the box
    # mask `all` (the lits default): nothing is kept zero
    ops = SmoothPredictOps()
    run("all", ops, "--prep_antialias", prep_mask="all")
    assert [c[3] for c in ops.smoothed] == [False, False]
    # the working arrays are prep's own: the same process_subject, the same plan
    entry = dict(prep.read_src_list(lst, "lits")[0], seg=None)
    plan = prep._Plan(entry, ("ct",), (2.5, 1.4, 2.0), (8, 8, 8), None, True)
    assert plan.radii == (3, 1, 0) and plan.sigmas == pytest.approx((0.75, 0.2, 0.0))
    # after the orient columns and before those of --blend
    _, _, t_all, _ = run("cols", SmoothPredictOps(), "--prep_antialias", "--blend", "gauss", prep_orient="RAS")
    assert t_all[0] == predict.CSV_HEADER + prep.ORIENT_COLUMNS + ["antialias"] + predict.CSV_BLEND_COLUMNS
    # a subject with nothing to filter: 0 0 0, the op is not called
    ops = SmoothPredictOps()
    _, _, t_up, said = run("up", ops, "--prep_antialias", prep_spacing="1,1,2")
    assert not hasattr(ops, "smoothed") and [r[-1] for r in t_up[1:]] == ["0 0 0"] * 2 and "anti-alias" not in said
